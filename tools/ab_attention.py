#!/usr/bin/env python3
"""A/B of two builds of the library over the attention stage (softmax + weighted sum, scores, the joined L2-norm backward):
    VQA_LIB=/path/to/libvqa_hip.so python tools/ab_attention.py dump FILE     every output of a fixed list of seeded cases
    python tools/ab_attention.py compare A B                                  byte equality per array, exit 1 on a difference
    VQA_LIB=/path/to/libvqa_hip.so python tools/ab_attention.py time          median ms per entry point at the workload's shape
dump / time run whatever library VQA_LIB names (default: the built one), each in a process of its own.  Outputs the wrappers
allocate are pre-filled with a sentinel, so an element a kernel leaves unwritten is compared too."""
import contextlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dl_vqa_amd import _lib, group_by_image, ops  # noqa: E402

SENTINEL = -12345.0
DEV = "cuda"


@contextlib.contextmanager
def sentinel_allocations():
    """torch.empty / torch.empty_like return sentinel-filled tensors while the cases run"""
    empty, empty_like = torch.empty, torch.empty_like
    torch.empty = lambda *a, **k: empty(*a, **k).fill_(SENTINEL)
    torch.empty_like = lambda *a, **k: empty_like(*a, **k).fill_(SENTINEL)
    try:
        yield
    finally:
        torch.empty, torch.empty_like = empty, empty_like


def randn(gen, *shape):
    return torch.randn(*shape, generator=gen, dtype=torch.float32).to(DEV)


def filled(*shape):
    return torch.full(shape, SENTINEL, dtype=torch.float32, device=DEV)


def grouping(gen, B, N):
    """B questions over images 0 .. N-2 in a shuffled order with every one of them asked; image N-1 is left unasked"""
    img = torch.cat([torch.arange(N - 1), torch.randint(0, N - 1, (B - (N - 1),), generator=gen)])
    img = img[torch.randperm(B, generator=gen)].to(torch.int32)
    order, offsets = group_by_image(img, N)
    return img.to(DEV), order.to(DEV), offsets.to(DEV)


def apply_cases(out, gen):
    for B, P, C, G in ((2, 676, 256, 2), (2, 70, 130, 3), (3, 100, 72, 1), (2, 17, 64, 4), (1, 65, 8, 2), (3, 1, 24, 3)):
        tag = f"apply B{B} P{P} C{C} G{G}"
        score, vn, dout = randn(gen, B, G, P), randn(gen, B, P, C), randn(gen, B, G * C)
        comb = filled(B, G * C)
        probs = ops.att_apply_fwd(score, vn, comb, G * C)
        out[f"{tag} fwd probs"], out[f"{tag} fwd out"] = probs, comb
        # the gather forms: Bq questions over N images
        N, Bq = B + 1, 2 * B + 1
        img, order, offsets = grouping(gen, Bq, N)
        gscore, gvn, gdout = randn(gen, Bq, G, P), randn(gen, N, P, C), randn(gen, Bq, G * C)
        gcomb = filled(Bq, G * C)
        gprobs = ops.att_apply_gather_fwd(gscore, gvn, img, gcomb, G * C)
        out[f"{tag} gather fwd probs"], out[f"{tag} gather fwd out"] = gprobs, gcomb
        bad = img.clone()
        bad[Bq // 2] = N                                            # that sample's rows stay at the sentinel
        bcomb = filled(Bq, G * C)
        bprobs = ops.att_apply_gather_fwd(gscore, gvn, bad, bcomb, G * C)
        assert bool((bcomb[Bq // 2] == SENTINEL).all()) and bool((bprobs[Bq // 2] == SENTINEL).all()), tag
        out[f"{tag} gather fwd probs, one index = N"], out[f"{tag} gather fwd out, one index = N"] = bprobs, bcomb
        if C % 4:
            continue                                                # the backward kernels read whole quads of channels
        for full in (True, False):                                  # with and without dvn and rowsum
            how = "dvn rowsum" if full else "bare"
            rowsum = filled(B, G) if full else None
            dscore, dvn = ops.att_apply_bwd(dout, G * C, probs, vn, rowsum=rowsum, want_dvn=full)
            out[f"{tag} bwd {how} dscore"] = dscore
            grow = filled(Bq, G) if full else None
            gdscore, gdvn = ops.att_apply_gather_bwd(gdout, G * C, gprobs, gvn, img, order, offsets, rowsum=grow)
            out[f"{tag} gather bwd {how} dscore"], out[f"{tag} gather bwd {how} dvn"] = gdscore, gdvn
            drow = filled(Bq, G) if full else None
            out[f"{tag} gather dscore {how}"] = ops.att_apply_gather_dscore(gdout, G * C, gprobs, gvn, img, rowsum=drow)
            if full:
                out[f"{tag} bwd dvn"], out[f"{tag} bwd rowsum"] = dvn, rowsum
                out[f"{tag} gather bwd rowsum"], out[f"{tag} gather dscore rowsum"] = grow, drow


def score_cases(out, gen):
    B, P = 2, 70
    # forward, one case per path: fp32 rows, fp32 general, fp32 general with qcat, bf16 fast, bf16 general
    fwd = [("fp32", 256, 1, False), ("fp32", 256, 2, False), ("fp32", 1024, 1, False), ("fp32", 1024, 2, False),
           ("fp32", 20, 3, False), ("fp32", 64, 2, True), ("bf16", 64, 2, False), ("bf16", 12, 2, False)]
    for dt, mid, G, cat in fwd:
        xld = 2 * mid if cat else mid
        xs = randn(gen, B * P, xld).relu_()
        xs = xs.to(torch.bfloat16) if dt == "bf16" else xs
        wx, bx = randn(gen, G, xld), randn(gen, G)
        qcat = randn(gen, B, mid) if cat else None
        for p in (0.0, 0.3):
            out[f"score fwd {dt} mid{mid} G{G} qcat{int(cat)} p{p}"] = ops.att_score_fwd(xs, wx, bx, B, P, p, 11, qcat=qcat)
    for mode in (0, 1, 2):
        for dt, mid, G in (("fp32", 64, 2), ("fp32", 20, 3), ("bf16", 64, 1)):
            xld = 2 * mid if mode == 2 else mid
            wx, vprime, qp, dscore = randn(gen, G, xld), randn(gen, B * P, mid), randn(gen, B, mid), randn(gen, B, G, P)
            for p in (0.0, 0.3):
                xs = randn(gen, B * P, xld).relu_()
                xs = xs.to(torch.bfloat16) if dt == "bf16" else xs
                dwx_part, dq_part, _ = ops.att_score_bwd(dscore, wx, xs, B, P, p, 12, mode=mode, vprime=vprime, qp=qp)
                tag = f"score bwd {dt} mode{mode} mid{mid} G{G} p{p}"
                out[f"{tag} xs"], out[f"{tag} dwx_part"], out[f"{tag} dq_part"] = xs, dwx_part, dq_part
    # two row splits with more than 256 column chunks (a second trip of the chunk walk); three splits, four glimpses
    for B, P, mid, G in ((2, 130, 1028, 1), (1, 257, 256, 4)):
        for mode in (0, 1, 2):
            xld = 2 * mid if mode == 2 else mid
            wx, vprime, qp, dscore = randn(gen, G, xld), randn(gen, B * P, mid), randn(gen, B, mid), randn(gen, B, G, P)
            for p in (0.0, 0.3):
                xs = randn(gen, B * P, mid).relu_()
                dwx_part, dq_part, _ = ops.att_score_bwd(dscore, wx, xs, B, P, p, 12, mode=mode, vprime=vprime, qp=qp)
                tag = f"score bwd fp32 B{B} P{P} mode{mode} mid{mid} G{G} p{p}"
                out[f"{tag} xs"], out[f"{tag} dwx_part"], out[f"{tag} dq_part"] = xs, dwx_part, dq_part


def grouped_cases(out, gen):
    N, B, P, M = 3, 7, 70, 4
    img, order, offsets = grouping(gen, B, N + 1)                   # the fourth image is the unasked one
    N += 1
    qrow = torch.randint(0, M, (B,), generator=gen).to(torch.int32).to(DEV)
    # mid 256: the register kernels ('+', '*'); 20, 1280 (two positions per wave) and 2052 (one): the general kernels
    for mid, G in ((256, 2), (20, 2), (256, 1), (20, 1), (256, 3), (256, 4), (20, 4), (1280, 2), (2052, 1)):
        for mode in (0, 1, 2):
            xld = 2 * mid if mode == 2 else mid
            vprime, qp, qtab = randn(gen, N * P, mid), randn(gen, B, mid), randn(gen, M, mid)
            wx, bx, dscore = randn(gen, G, xld), randn(gen, G), randn(gen, B, G, P)
            tag = f"grouped mid{mid} mode{mode}" if G == 2 else f"grouped mid{mid} G{G} mode{mode}"
            out[f"{tag} fwd"] = ops.att_score_grouped_fwd(vprime, qp, wx, bx, order, offsets, N, B, P, mode)
            out[f"{tag} pairs fwd"] = ops.att_score_grouped_pairs_fwd(vprime, qtab, qrow, wx, bx, order, offsets, N, B, P, mode)
            for p in (0.0, 0.3):
                out[f"{tag} drop fwd p{p}"] = ops.att_score_grouped_drop_fwd(vprime, qp, wx, bx, order, offsets, N, B, P, mode, p, 13)
                dv, dq, dw, _ = ops.att_score_grouped_bwd(dscore, vprime, qp, wx, order, offsets, N, B, P, mode, p, 13)
                out[f"{tag} bwd p{p} dvprime"], out[f"{tag} bwd p{p} dq_part"], out[f"{tag} bwd p{p} dwx_part"] = dv, dq, dw


def other_cases(out, gen):
    B, P, C, G = 2, 70, 64, 2
    dout, probs = randn(gen, B, G * C), torch.softmax(randn(gen, B, G, P), -1)
    dv_in, vn, norm = randn(gen, B * P, C), randn(gen, B, P, C), randn(gen, B * P).abs_() + 0.5
    for p_v, p in ((0.0, 0.0), (0.3, 0.2)):
        out[f"l2norm_bwd_joined G{G} p_v{p_v} p{p}"] = ops.l2norm_bwd_joined(dout, G * C, probs, dv_in, p_v, 14, vn, norm, p, 15)
    x = randn(gen, 8 * 513 + 5)
    for p in (0.0, 0.3):
        out[f"dropout_to_bf16 p{p}"] = ops.dropout_to_bf16(x, p, 16)


def dump(path):
    gen = torch.Generator().manual_seed(20240607)
    out = {}
    with sentinel_allocations():
        for cases in (apply_cases, score_cases, grouped_cases, other_cases):
            cases(out, gen)
    torch.cuda.synchronize()
    arrays = {k: (v.view(torch.int16) if v.dtype == torch.bfloat16 else v).cpu().numpy() for k, v in out.items()}
    np.savez(path, **arrays)
    print(f"{len(arrays)} arrays from {_lib.LIB_PATH} -> {path}")


def compare(a, b):
    A, B = np.load(a), np.load(b)
    names = sorted(set(A.files) | set(B.files))
    differ = 0
    for k in names:
        same = k in A.files and k in B.files and A[k].dtype == B[k].dtype and A[k].shape == B[k].shape and A[k].tobytes() == B[k].tobytes()
        differ += not same
        print(f"{'equal ' if same else 'DIFFER'} {k}" + (f" {A[k].shape}" if same else ""))
    print(f"{len(names)} arrays, {differ} differ")
    return 1 if differ else 0


def median_ms(f, warmup=20, n=200):
    for _ in range(warmup):
        f()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for s, e in ev:
        s.record()
        f()
        e.record()
    torch.cuda.synchronize()
    return float(np.median([s.elapsed_time(e) for s, e in ev]))


def time_entry_points():
    """the workload's attention shape in train mode: B = 256, P = 676, C = 256, mid = 1024, G = 2"""
    gen = torch.Generator().manual_seed(7)
    B, P, C, mid, G, p = 256, 676, 256, 1024, 2, 0.5
    N = B // 8                                                      # the gather forms: 8 questions per image
    score, vn, dout = randn(gen, B, G, P), randn(gen, B, P, C), randn(gen, B, G * C)
    comb, rowsum = filled(B, G * C), filled(B, G)
    probs = ops.att_apply_fwd(score, vn, comb, G * C)
    img = (torch.arange(B) % N).to(torch.int32)
    order, offsets = group_by_image(img, N)
    img, order, offsets = img.to(DEV), order.to(DEV), offsets.to(DEV)
    xs, wx, bx = randn(gen, B * P, mid).relu_(), randn(gen, G, mid), randn(gen, G)
    xs16 = xs.to(torch.bfloat16)
    dv_in, norm = randn(gen, B * P, C), randn(gen, B * P).abs_() + 0.5
    vprime, qp = randn(gen, N * P, mid), randn(gen, B, mid)         # the grouped score forms: 32 images x 8 questions
    runs = {
        "att_apply_fwd": lambda: ops.att_apply_fwd(score, vn, comb, G * C),
        "att_apply_bwd (no dvn)": lambda: ops.att_apply_bwd(dout, G * C, probs, vn, rowsum=rowsum, want_dvn=False),
        "att_apply_gather_fwd": lambda: ops.att_apply_gather_fwd(score, vn[:N], img, comb, G * C),
        "att_apply_gather_bwd": lambda: ops.att_apply_gather_bwd(dout, G * C, probs, vn[:N], img, order, offsets, rowsum=rowsum),
        "att_score_fwd fp32": lambda: ops.att_score_fwd(xs, wx, bx, B, P, p, 1),
        "att_score_fwd bf16": lambda: ops.att_score_fwd(xs16, wx, bx, B, P, p, 1),
        "att_score_bwd fp32": lambda: ops.att_score_bwd(probs, wx, xs, B, P, p, 1),
        "att_score_grouped_drop_fwd": lambda: ops.att_score_grouped_drop_fwd(vprime, qp, wx, bx, order, offsets, N, B, P, 0, p, 1),
        "att_score_grouped_bwd": lambda: ops.att_score_grouped_bwd(probs, vprime, qp, wx, order, offsets, N, B, P, 0, p, 1),
        "l2norm_bwd_joined": lambda: ops.l2norm_bwd_joined(dout, G * C, probs, dv_in, p, 2, vn, norm, 0.0, 3),
    }
    print(f"library {_lib.LIB_PATH}")
    for name, f in runs.items():
        print(f"{name:26s} {median_ms(f):8.4f} ms")


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    if mode == "dump" and len(sys.argv) == 3:
        dump(sys.argv[2])
    elif mode == "compare" and len(sys.argv) == 4:
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    elif mode == "time" and len(sys.argv) == 2:
        time_entry_points()
    else:
        sys.exit(__doc__)
