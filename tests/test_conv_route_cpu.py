"""CPU: the conv blocks' kernel routes (Engine.conv_routes) and the launches both passes make from them.

tests/conv_route_trace.py records every library call of _image_encoder and _conv_bwd on CPU tensors; the golden file holds
the traces of the commit before the routes existed (its hash is in the file), when forward and backward each derived the
decision on their own.  Every trace must be reproduced exactly: same entry points, same order, same scalars, same dataflow.
The route kinds per block are written out by hand below."""
import json
import os

import pytest

from dl_vqa_amd import ops
from dl_vqa_amd.engine import Engine
from tests import conv_route_trace as T

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_route_traces.json")) as _f:
    GOLDEN = json.load(_f)["traces"]

# case -> the route of every block, keep=True: kind (+x3: on the split kernels, +pdg: backward-data on the fp32 patch kernel)
KINDS = {
    "fp32_tiny": ["conv32", "conv32", "conv32"],                    # 8 output channels: no dedicated first block
    "fp32_full": ["conv0", "conv32+pdg", "conv32"],                 # 128-channel input stays on the implicit-GEMM dgrad
    "fp32_full_pdgrad0": ["conv0", "conv32", "conv32"],
    "fp32_full_pdgrad2": ["conv0", "conv32+pdg", "conv32+pdg"],
    "x3_mixed96": ["conv0", "conv32+x3", "conv32"],                 # 47 x 47 has the split kernels, 22 x 22 has not
    "x3_full224": ["conv0", "conv32+x3", "conv32+x3"],
    "x3_pack_in224": ["conv32", "conv32", "conv32+x3"],             # block 2 packs its own input: block 1 is not split
    "bf16_full": ["conv0", "pconv", "pconv"],
    "bf16_full_pconv0": ["conv0", "conv16", "conv16"],
    "bf16_64_64_128": ["conv0", "conv16", "conv16"],                # no patch wgrad for block 1: every block falls back
    "k5": ["convk", "convk"],
    "stride2": ["conv32", "conv32"],                                # the dedicated first block is stride 1 only
    "fp16_full": ["conv0", "conv32+pdg", "conv32"],
    "fp16_tiny": ["conv32", "conv32", "conv32"],
}
# case -> (src of block 0, out of every block, dy of every block, dx of every block with need_dx)
LAYOUTS = {
    "fp32_tiny": ("nhwc32", ["nhwc32"] * 3, ["nhwc32"] * 3, ["nhwc32"] * 3),
    "x3_mixed96": ("nchw", ["x3", "nhwc32", "nhwc32"], ["nhwc32"] * 3, ["nchw", "nhwc32", "nhwc32"]),
    "x3_full224": ("nchw", ["x3", "x3", "nhwc32"], ["nhwc32"] * 3, ["nchw", "nhwc32", "nhwc32"]),
    "bf16_full": ("nchw", ["c16", "c16", "nhwc32"], ["nhwc16", "c16", "c16"], ["nchw", "nhwc16", "c16"]),
    "bf16_full_pconv0": ("nchw", ["nhwc16", "nhwc16", "nhwc32"], ["nhwc16"] * 3, ["nchw", "nhwc16", "nhwc16"]),
}


def _label(r):
    return r.kind + ("+x3" if r.x3 else "") + ("+pdg" if r.pdg else "")


@pytest.mark.parametrize("tid,name,keep,need_dx", T.trace_ids(), ids=[t[0] for t in T.trace_ids()])
def test_trace_equals_the_parents(tid, name, keep, need_dx):
    t = T.trace(name, keep, need_dx)
    # through JSON: the golden file's lists and numbers
    got = json.loads(json.dumps({k: t[k] for k in ("forward", "backward") if k in t}))
    assert got["forward"] == GOLDEN[tid]["forward"]
    assert got.get("backward") == GOLDEN[tid].get("backward")
    routes = t["enc"].routes
    # without backward no block takes the patch backward-data kernel or packs weights for it
    assert [_label(r) for r in routes] == (KINDS[name] if keep else [k.replace("+pdg", "") for k in KINDS[name]])
    assert keep or not any(r.need_wd for r in routes)
    # only x3_pack_in224's last block meets a producer that could not write the x3-packed form
    assert [r.pack_in for r in routes] == [name == "x3_pack_in224" and l == 2 for l in range(len(routes))]
    assert any(c[0] == "vqa_x3_pack" for c in got["forward"]) == (name == "x3_pack_in224")
    assert t["enc"].fast0 == (KINDS[name][0] == "conv0") and t["enc"].use_pc == ("pconv" in KINDS[name])
    if keep:
        assert [w is not None for w in t["enc"].wds] == [r.need_wd or r.pdg for r in routes]
        assert routes[0].dx == (None if not need_dx else "nchw" if routes[0].kind == "conv0" else "nhwc32")


@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_route_layouts(name):
    dtype, channels, S, rest = T.CASES[name]
    eng = Engine(T.engine_cfg(channels), 40, dtype)
    with T.recorded(rest.get("env", {})) as log:
        routes = eng.conv_routes((rest.get("B", 2), 3, S, S), True, True)
    src0, out, dy, dx = LAYOUTS[name]
    assert log == []
    assert [r.src for r in routes] == [src0] + out[:-1]
    assert [r.out for r in routes] == out and [r.dy for r in routes] == dy and [r.dx for r in routes] == dx
    assert [r.pack_in for r in routes] == [False] * 3       # every producer here writes the form its consumer reads
    H = S
    for l, r in enumerate(routes):
        assert r.x_shape == (rest.get("B", 2), H, H, 3 if src0 == "nchw" and l == 0 else 4 if l == 0 else channels[l])
        assert r.Co == channels[l + 1]
        H = (H - 2) // 2


@pytest.mark.parametrize("name,knobs", [("fp32_full", dict(VQA_PDGRAD="0")), ("fp32_full_pdgrad0", dict(VQA_PDGRAD="2")),
                                        ("bf16_full", dict(VQA_PCONV="0")), ("bf16_full_pconv0", dict(VQA_PCONV="1"))])
def test_backward_ignores_knobs_changed_after_the_forward(name, knobs):
    t = T.trace(name, True, True, between=lambda eng: os.environ.update(knobs))
    assert json.loads(json.dumps(t["backward"])) == GOLDEN[f"{name}/dx1"]["backward"]


@pytest.mark.parametrize("name", ["fp32_full", "x3_mixed96", "x3_full224", "bf16_full", "bf16_full_pconv0", "k5", "stride2"])
def test_backward_asks_nothing_again(name, monkeypatch):
    """_conv_bwd reads the routes: no *_supported query and no _x3_layer."""
    def between(eng):
        def asked(*a, **k):
            raise AssertionError("the backward asked for a decision the forward made")
        monkeypatch.setattr(eng, "_x3_layer", asked)
        for fn in [n for n in dir(ops) if n.endswith("_supported")]:
            monkeypatch.setattr(ops, fn, asked)
    t = T.trace(name, True, True, between=between)
    assert json.loads(json.dumps(t["backward"])) == GOLDEN[f"{name}/dx1"]["backward"]


def test_bf16_without_the_dedicated_first_block_raises_before_any_launch():
    assert not ops.conv0_supported(3, 66, 66, 64, 1)        # W % 4 != 0
    eng = Engine(T.engine_cfg(T.FULL), 40, "bf16")
    P, _, v = T.inputs(eng, 2, 66)
    with T.recorded({}) as log:
        with pytest.raises(ValueError, match="dedicated first-block kernel"):
            eng._image_encoder(P, v, True)
    assert log == []
