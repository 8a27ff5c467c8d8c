"""Times the input-image gradient: vqa_conv0_dgrad alone at configs[1] (B=256, 224 x 224, fp32 pooled gradient) and
configs[3] (B=512, 448 x 448, bf16 pooled gradient), with the achieved TB/s against the bytes it must move, and one
train step (forward + loss + backward) of the north-star model at configs[1] with and without v.requires_grad.

    python tools/kbench_input_grad.py [--iters N] [--no-step]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters


def kernel(B, S, dp_dtype, iters):
    from dl_vqa_amd import ops
    Ci, Co = 3, 64
    Hp = Wp = (S - 2) // 2
    g = torch.Generator(device="cuda").manual_seed(1)
    dp = torch.randn(B, Hp, Wp, Co, device="cuda", generator=g).to(dp_dtype)
    am = torch.randint(0, 5, (B, Hp, Wp, Co), device="cuda", generator=g, dtype=torch.uint8)
    w = torch.randn(Co, Ci, 3, 3, device="cuda", generator=g)
    ms = timed(lambda: ops.conv0_dgrad(dp, am, w, (B, Ci, S, S)), iters)
    nbytes = dp.numel() * dp.element_size() + am.numel() + B * Ci * S * S * 4
    del dp, am
    torch.cuda.empty_cache()
    return dict(B=B, S=S, dpooled=str(dp_dtype).split(".")[-1], ms=round(ms, 4), GB=round(nbytes / 1e9, 3),
                TBps=round(nbytes / ms / 1e9, 2))


def step(B, S, iters):
    from dl_vqa_amd import VqaNet
    from dl_vqa_amd.train import soft_ce_loss_and_score
    from oracle import vqa_oracle as O
    from tests.golden_util import full_cfg
    torch.manual_seed(1)
    m = VqaNet(full_cfg(3000), 15000).cuda().train()
    v, q, a_idx, a_val, _, _, ql = O.synthetic_batch(B, S, 14, 15000, 3000, seed=2)
    v, q, ql, a_idx, a_val = (t.cuda() for t in (v, q, ql, a_idx, a_val))
    out = {}
    for want in (False, True):
        vin = v.clone().requires_grad_(want)

        def one():
            m.zero_grad(set_to_none=True)
            vin.grad = None
            y = m(vin, q, ql)
            soft_ce_loss_and_score(y, a_idx, a_val)[0].backward()
        out["with_v_grad" if want else "without_v_grad"] = round(timed(one, iters), 3)
    out["difference_ms"] = round(out["with_v_grad"] - out["without_v_grad"], 3)
    return dict(B=B, S=S, **out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    res = {"kernel": [kernel(256, 224, torch.float32, a.iters), kernel(512, 448, torch.bfloat16, a.iters)]}
    if not a.no_step:
        res["step"] = step(256, 224, max(a.iters // 2, 5))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
