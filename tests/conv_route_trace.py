"""Launch traces of the image encoder and its backward, made without a GPU.

Engine._image_encoder, _encoder_saved and _conv_bwd run on CPU tensors with ops.call / ops.stream / ops.workspace /
ops.ptr replaced: every library entry point they would launch is recorded as [name, arg, ...] and none is made (the
library's *_supported and *_workspace_bytes functions make no HIP call and are asked as usual).  Pointers become symbols in
order of first appearance, "t<k>+<byte offset from the storage base>" (None: NULL); every tensor whose pointer was seen is
held until the trace ends, so no address is ever reused and the symbols pin the dataflow: which buffer feeds which call.
Floats are rounded to 6 places, the stream is 0.

tests/golden/conv_route_traces.json holds the traces of the commit BEFORE the conv routes were introduced, written by
running this file on a checkout of that commit:  python -m tests.conv_route_trace <out.json> <commit hash>.
It only uses what that commit's engine has too: the three signatures above and the namespace _image_encoder returns.
"""
import contextlib
import json
import os
import sys
import types

import torch

from dl_vqa_amd import _lib, ops
from dl_vqa_amd.engine import Engine
from tests.golden_util import tiny_cfg

FULL, TINY = [3, 64, 128, 256], [3, 8, 16, 32]
# name -> (compute_dtype, channels, S, the rest: B, kernel_size, stride, vdtype, env)
CASES = {
    "fp32_tiny": ("fp32", TINY, 32, {}),
    "fp32_full": ("fp32", FULL, 64, {}),
    "fp32_full_pdgrad0": ("fp32", FULL, 64, dict(env={"VQA_PDGRAD": "0"})),
    "fp32_full_pdgrad2": ("fp32", FULL, 64, dict(env={"VQA_PDGRAD": "2"})),
    "x3_mixed96": ("fp32x3", FULL, 96, {}),
    "x3_full224": ("fp32x3", FULL, 224, dict(B=1)),
    "x3_pack_in224": ("fp32x3", [3, 16, 64, 128], 224, dict(B=1)),      # generic first block; only block 2 is split
    "bf16_full": ("bf16", FULL, 64, {}),
    "bf16_full_pconv0": ("bf16", FULL, 64, dict(env={"VQA_PCONV": "0"})),
    "bf16_64_64_128": ("bf16", [3, 64, 64, 128], 64, {}),
    "k5": ("fp32", [3, 8, 16], 40, dict(kernel_size=5)),
    "stride2": ("fp32", [3, 64, 128], 64, dict(stride=2)),
    "fp16_full": ("fp32", FULL, 64, dict(vdtype=torch.float16)),
    "fp16_tiny": ("fp32", TINY, 32, dict(vdtype=torch.float16)),
}
KEEP_FALSE = ("fp32_full", "x3_full224", "bf16_full")       # once more with keep=False: forward trace only


def trace_ids():
    """(trace id, case, keep, need_dx) of every trace of the golden file."""
    ids = [(f"{name}/dx{int(dx)}", name, True, dx) for name in CASES for dx in (False, True)]
    return ids + [(f"{name}/nokeep", name, False, False) for name in KEEP_FALSE]


def engine_cfg(channels, kernel_size=3, stride=1):
    cfg = tiny_cfg(dict(bidirectional=True, stride=stride, do_option="+", kernel_size=kernel_size))
    cfg["image"]["num_channels"] = list(channels)
    return cfg


@contextlib.contextmanager
def recorded(env):
    """ops' four doors to the library replaced by recorders and the conv knobs set to `env` (unset otherwise); yields the log."""
    log, symbols, held, ws = [], {}, [], [None]

    def ptr(t):
        if t is None:
            return None
        held.append(t)
        base = t.untyped_storage().data_ptr()
        return f"{symbols.setdefault(base, f't{len(symbols)}')}+{t.data_ptr() - base}"

    def call(name, *args):
        log.append([name] + [round(a, 6) if isinstance(a, float) else a for a in args])

    def workspace(nbytes, device):          # grows like ops.workspace, from nothing in every trace
        if ws[0] is None or ws[0].numel() * 4 < nbytes:
            ws[0] = torch.empty(ops._workspace_floats(nbytes), dtype=torch.float32)
        return ws[0]

    saved = {k: getattr(ops, k) for k in ("call", "ptr", "stream", "workspace")}
    # no VQA_* knob but the case's own is in force: the library reads its knobs once per process, other tests may have set some
    saved_env = {k: os.environ.pop(k) for k in list(os.environ) if k.startswith("VQA_") and k != "VQA_LIB"}
    os.environ.update(env)
    _lib.load().vqa_reload_knobs()
    ops.call, ops.ptr, ops.stream, ops.workspace = call, ptr, (lambda: 0), workspace
    try:
        yield log
    finally:
        for k, f in saved.items():
            setattr(ops, k, f)
        for k in [k for k in os.environ if k.startswith("VQA_") and k != "VQA_LIB"]:
            del os.environ[k]
        os.environ.update(saved_env)
        _lib.load().vqa_reload_knobs()


def inputs(eng, B, S, vdtype=torch.float32):
    """(P, Gr, v): conv parameters, their gradient buffers and an image batch [B,C,S,S] for eng, on the CPU."""
    ch, P = eng.channels, {}
    for l in range(eng.L):
        P[f"image.conv{l}.weight"] = torch.zeros(ch[l + 1], ch[l], eng.ks, eng.ks)
        P[f"image.conv{l}.bias"] = torch.zeros(ch[l + 1])
    return P, {k: torch.zeros_like(t) for k, t in P.items()}, torch.zeros(B, ch[0], S, S, dtype=vdtype)


def trace(name, keep=True, need_dx=False, between=None):
    """The trace of one case: dict(forward=[...], backward=[...] (with keep), enc=what _image_encoder returned,
    engine=the Engine).  between(engine): called after the forward and before the backward."""
    dtype, channels, S, rest = CASES[name]
    rest = dict(rest)
    B, vdtype, env = rest.pop("B", 2), rest.pop("vdtype", torch.float32), rest.pop("env", {})
    with recorded(env) as log:
        eng = Engine(engine_cfg(channels, **rest), 40, dtype)
        P, Gr, v = inputs(eng, B, S, vdtype)
        out = dict(engine=eng, forward=log)
        out["enc"] = enc = eng._image_encoder(P, v, keep, need_dx)
        if not keep:
            return out
        out["forward"], n = log[:], len(log)
        ctx = types.SimpleNamespace(**eng._encoder_saved(enc, None, 0.0, need_dx, v))
        if between is not None:
            between(eng)
        # the pooled gradient as the L2-norm backward hands it over: bf16 on the bf16 path, channel-blocked for the patch kernels
        Bo, Ho, Wo, Co = enc.out.shape
        if eng.bf16 and enc.use_pc:
            dP = torch.zeros(Bo, Co // 16, Ho, Wo, 16, dtype=torch.bfloat16)
        else:
            dP = torch.zeros(Bo, Ho, Wo, Co, dtype=torch.bfloat16 if eng.bf16 else torch.float32)
        eng._conv_bwd(P, ctx, dP, Gr)
        out["backward"] = log[n:]
        return out


if __name__ == "__main__":
    path, parent = sys.argv[1:]
    traces = {}
    for tid, name, keep, need_dx in trace_ids():
        t = trace(name, keep, need_dx)
        traces[tid] = {k: t[k] for k in ("forward", "backward") if k in t}
    with open(path, "w") as f:
        f.write('{"parent": %s,\n "traces": {\n' % json.dumps(parent))
        f.write(",\n".join("  %s: %s" % (json.dumps(k), json.dumps(t, separators=(",", ":"))) for k, t in traces.items()))
        f.write("\n }}\n")
