#!/usr/bin/env python3
"""One timing sample (ms per launch) of the first conv block's kernels and of one inner block's forward, at the benchmark's
shapes (B = 256, 224 x 224; the bf16 path at 448 x 448 with --size 448):
    python tools/kbench_conv0.py [--batch 256] [--size 224] [--iters 20]
VQA_LIB selects the library, so two builds can be sampled alternately, one process per sample.
tools/kbench.py and tools/kbench_bf16.py time their whole model at one size in every process and have no entry for the C16
forward from a __half image or for conv0_wgrad_bf16; this file holds just the six kernels that share the first block's
pool pick and helpers, so that a sample takes seconds and many can be alternated."""
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
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    B, S, dev, bf16 = args.batch, args.size, "cuda:0", torch.bfloat16

    def run(name, fn):
        print(f"{name:28s} {timeit(fn, args.iters):9.4f} ms", flush=True)

    img = torch.randn(B, 3, S, S, device=dev)
    imgh = img.half()
    w0, b0 = torch.randn(64, 3, 3, 3, device=dev) * 0.2, torch.zeros(64, device=dev)
    p0, a0 = ops.conv0_fwd(img, w0, b0)
    run("conv0_fwd fp32", lambda: ops.conv0_fwd(img, w0, b0))
    run("conv0_fwd C16 half image", lambda: ops.conv0_fwd(imgh, w0, b0, out_dtype=bf16, bf16_mfma=True, out_c16=True))
    dp0, dw0, db0 = torch.randn_like(p0), torch.empty_like(w0), torch.empty_like(b0)
    run("conv0_wgrad", lambda: ops.conv0_wgrad(img, dp0, a0, dw0, db0))
    dp0h = dp0.to(bf16)
    run("conv0_wgrad_bf16", lambda: ops.conv0_wgrad_bf16(imgh, dp0h, a0, dw0, db0))
    # block 1: 64 -> 128 channels on the pooled map of block 0
    w1, b1 = torch.randn(128, 64, 3, 3, device=dev) / 24.0, torch.zeros(128, device=dev)
    wf, _ = ops.conv_pack_weights(w1, 64)
    run("conv1 fp32 implicit-GEMM fwd", lambda: ops.conv_fwd(p0, wf, b1, 1, tag=1))
    wfp, _ = ops.pconv_pack_weights(w1)
    xc = ops.to_c16(p0.to(bf16))
    run("conv1 bf16 patch fwd", lambda: ops.pconv_fwd(xc, wfp, b1, 128, out_dtype=bf16, tag=1))


if __name__ == "__main__":
    main()
