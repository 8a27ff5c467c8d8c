"""Times the answer ranking: one launch of ops.softmax_topk against torch.softmax followed by torch.topk on the same logits,
at the headline and stress shapes of BASELINE.json (B=256, A=1000, k=5 and B=1024, A=3000, k=10).

A sample is the device time of `--calls` back-to-back calls between two events, divided by the calls; the two sides alternate
sample by sample in one process, and the median of `--rounds` samples per side is reported with the extremes.  Before the
timing the two sides are compared on the timed logits: the same indices (the rows are checked to hold no ties) and
probabilities within 4e-6 relative.

    python tools/kbench_topk.py [--calls N] [--rounds R]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(256, 1000, 5), (1024, 3000, 10)]


def sample(fn, calls):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(calls):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / calls          # microseconds per call


def shape(B, A, k, calls, rounds):
    from dl_vqa_amd import ops
    g = torch.Generator(device="cuda").manual_seed(B + A)
    x = torch.randn(B, A, device="cuda", generator=g) * 3

    def ours():
        return ops.softmax_topk(x, k)

    def pair():
        return torch.topk(torch.softmax(x, dim=1), k, dim=1)

    idx, prob = ours()
    val, tidx = pair()
    ties = int((torch.sort(x, dim=1).values.diff(dim=1) == 0).sum())
    same_idx = bool(torch.equal(idx.long(), tidx)) if ties == 0 else None
    rel = float(((prob - val).abs() / val).max()) if same_idx else None
    for fn in (ours, pair):                           # warm-up: code objects, the allocator's blocks
        sample(fn, calls)
    t = {"softmax_topk": [], "torch_softmax_topk": []}
    for _ in range(rounds):
        t["softmax_topk"].append(sample(ours, calls))
        t["torch_softmax_topk"].append(sample(pair, calls))
    out = dict(B=B, A=A, k=k, tied_entries=ties, same_indices=same_idx, max_rel_prob_diff=rel)
    for name, v in t.items():
        out[name + "_us"] = dict(median=round(statistics.median(v), 2), min=round(min(v), 2), max=round(max(v), 2))
    out["ratio_torch_over_ours"] = round(out["torch_softmax_topk_us"]["median"] / out["softmax_topk_us"]["median"], 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=15)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kbench_topk needs an MI355X; there is nothing to time on the CPU")
    print(json.dumps({"device": torch.cuda.get_device_name(0), "calls_per_sample": a.calls, "rounds": a.rounds,
                      "shapes": [shape(B, A, k, a.calls, a.rounds) for B, A, k in SHAPES]}))


if __name__ == "__main__":
    main()
