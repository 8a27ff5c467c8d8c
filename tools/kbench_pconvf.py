#!/usr/bin/env python3
"""One timing sample (ms per launch) of the fp32 patch backward-data kernel (csrc/conv_patch_f32.hip) at block 1's shape,
64 -> 128 channels on the pooled map of block 0:
    python tools/kbench_pconvf.py [--batch 256] [--hw 111] [--iters 20]        # the 224 x 224 benchmark; --batch 128 --hw 223: 448 x 448
VQA_LIB selects the library, so two builds can be sampled alternately, one process per sample.  The arg-max bytes are a
forward kernel's on random activations; the line also carries a checksum of the output's bits (the sum of its words as
integers), which two builds that compute the same thing must share."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dl_vqa_amd import ops  # noqa: E402


def timeit(fn, iters):
    fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--hw", type=int, default=111)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    B, S, Ci, Co, dev = args.batch, args.hw, 64, 128, "cuda:0"
    assert ops.pconvf_supported(S, S, Ci, Co)
    torch.manual_seed(0)
    x = torch.randn(B, S, S, Ci, device=dev)
    w, b = torch.randn(Co, Ci, 3, 3, device=dev) / 24.0, torch.zeros(Co, device=dev)
    wf, _ = ops.conv_pack_weights(w, Ci, need_wd=False)
    pooled, am = ops.conv_fwd(x, wf, b, 1, tag=1)
    dp = torch.randn_like(pooled)
    del wf, pooled
    wimg = ops.pconvf_pack_weights(w)
    dx = torch.empty_like(x)
    ms = timeit(lambda: ops.pconvf_dgrad(dp, am, wimg, tuple(x.shape), tag=1, out=dx), args.iters)
    flops = 2.0 * B * (S - 2) * (S - 2) * Ci * Co * 9
    bits = int(dx.view(torch.int32).sum(dtype=torch.int64))
    print(f"pconvf_dgrad B={B} {S}x{S} {Ci}->{Co} {ms:9.4f} ms  {flops / ms * 1e-9:6.1f} TFLOP/s  bits {bits}", flush=True)


if __name__ == "__main__":
    main()
