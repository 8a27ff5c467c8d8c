"""Adam over a table of segments (vqa_adam_segments, FusedAdam(groups=...)) against what it stands beside or replaces.

    python tools/kbench_adam_segments.py [--out profiles/adam_segments_bench.json] [--reps 9] [--iters 400]

North-star architecture (224 x 224, A = 1000, V = 5000), fp32.  Three comparisons, each with its two sides alternating window
by window in this one process, HIP events on the stream, the figure the median over --reps windows (every window's time is
reported, so the spread is there to read):
  (a) vqa_adam_segments with ONE segment over the model's whole flat buffer against vqa_adam on the same buffers (prebuilt
      table, the same Python call path on both sides).  The bar: the segment kernel's median is not above vqa_adam's by more
      than vqa_adam's own window-to-window spread (max - min) in this run.
  (b) FusedAdam.step() with the image.* parameters grad-less, as after run_batch_features: groups=[image frozen] (the table
      leaves the range out) against the legacy optimiser's skip path (clone value and moments of every skipped parameter,
      update the whole buffer, copy back).
  (c) the whole feature-train step of tools/bench_feature_train.py case (a) (256 questions on 256 distinct rows of a 256-row
      bank, train mode) with the legacy FusedAdam against groups=[image frozen], on one model with two optimisers.
One JSON line on stdout (and in --out).  Run it under a time limit; it starts no further process.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_multi_question import _window  # noqa: E402  (the timing window)

S, T, A, V, B = 224, 14, 1000, 5000, 256
HBM_PEAK_GBPS = 8000.0
LR = 1e-4


def _dist(ms, digits=4):
    return dict(median_ms=round(statistics.median(ms), digits), min_ms=round(min(ms), digits), max_ms=round(max(ms), digits),
                windows_ms=[round(x, digits) for x in ms])


def _alternate(sides, reps, iters, warmup=3):
    """{name: [ms per call of every window]}, the sides taking turns window by window."""
    import torch
    for _ in range(warmup):
        for fn in sides.values():
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in sides}
    for _ in range(reps):
        for k, fn in sides.items():
            t[k].append(_window(fn, iters))
    return t


def kernel_against_vqa_adam(n, reps, iters):
    import torch
    from dl_vqa_amd import _lib, ops
    g = torch.Generator().manual_seed(1)
    p, gr = torch.randn(n, generator=g).cuda(), (torch.randn(n, generator=g) * 1e-2).cuda()
    m, v = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    table = ops.adam_segment_table([(0, n, LR, 0.9, 0.999, 1e-8, 0.0, 10, 0)])

    def segments():
        _lib.call("vqa_adam_segments", p.data_ptr(), gr.data_ptr(), m.data_ptr(), v.data_ptr(), n, table, 1, 1.0, _lib.stream())

    t = _alternate({"vqa_adam": lambda: ops.adam(p, gr, m, v, LR, 10), "vqa_adam_segments": segments}, reps, iters)
    a, s = _dist(t["vqa_adam"]), _dist(t["vqa_adam_segments"])
    nbytes = 28 * n                                         # p, m, v read and written, g read
    for d in (a, s):
        d["GBps"] = round(nbytes / d["median_ms"] / 1e6, 1)
        d["fraction_of_8TBps_hbm_peak"] = round(d["GBps"] / HBM_PEAK_GBPS, 3)
    spread = a["max_ms"] - a["min_ms"]
    return dict(n=n, bytes=nbytes, vqa_adam=a, vqa_adam_segments=s, vqa_adam_window_spread_ms=round(spread, 4),
                segments_minus_adam_ms=round(s["median_ms"] - a["median_ms"], 4),
                bar="segments median - vqa_adam median <= vqa_adam's (max - min) over its windows",
                within_bar=bool(s["median_ms"] - a["median_ms"] <= spread))


def _model():
    import torch
    from dl_vqa_amd import VqaNet
    from tests.golden_util import full_cfg
    torch.manual_seed(1)
    return VqaNet(full_cfg(A), V).cuda().train()


def step_without_image(m, reps, iters):
    """opt.step() alone: gradients as run_batch_features leaves them (views of the flat buffer, none for image.*)."""
    import torch
    from dl_vqa_amd.train import FusedAdam
    flat_p, flat_g, offsets = m.flat_buffers()
    flat_g.copy_(torch.randn(flat_g.numel(), generator=torch.Generator().manual_seed(2)).cuda() * 1e-3)
    views = m._grad_views()
    for n, p in m.named_parameters():
        p.grad = None if n.startswith("image.") else views[n]
    legacy = FusedAdam(m, lr=LR)
    grouped = FusedAdam(m, lr=LR, groups=[{"params": "image", "frozen": True}])
    t = _alternate({"legacy_skip_path": legacy.step, "groups_image_frozen": grouped.step}, reps, iters)
    lo, hi = m.group_range("image")
    segs, _ = grouped._segments(flat_g)
    out = dict(flat_floats=flat_p.numel(), image_floats=hi - lo,
               image_parameters=sum(1 for n in offsets if n.startswith("image.")), segments=len(segs),
               legacy_skip_path=_dist(t["legacy_skip_path"]), groups_image_frozen=_dist(t["groups_image_frozen"]))
    out["saved_ms"] = round(out["legacy_skip_path"]["median_ms"] - out["groups_image_frozen"]["median_ms"], 4)
    for p in m.parameters():
        p.grad = None
    return out


def feature_train_step(m, reps, iters):
    """tools/bench_feature_train.py case (a): forward_features, fused loss, backward, step -- two optimisers, one model."""
    import torch
    from dl_vqa_amd.train import FusedAdam, run_batch_features
    from oracle import vqa_oracle as O
    v, q, a_idx, a_val, a_len, idx, ql = O.synthetic_batch(B, S, T, V, A, seed=2)
    q, ql, a_idx, a_val = q.cuda(), ql.cuda(), a_idx.cuda(), a_val.cuda()
    image_index = torch.arange(B)
    m.eval()
    feats = m.encode_images(v.cuda(), with_vprime=False)
    m.train()
    nov = (None, q, a_idx, a_val, a_len, idx, ql)
    opts = {"legacy": FusedAdam(m, lr=LR), "groups_image_frozen": FusedAdam(m, lr=LR, groups=[{"params": "image", "frozen": True}])}

    def step(opt):
        loss = run_batch_features(m, nov, A, feats, image_index)[0]
        opt.zero_grad()
        loss.backward()
        opt.step()

    t = _alternate({k: (lambda o=o: step(o)) for k, o in opts.items()}, reps, iters, warmup=2)
    out = {k: _dist(ms, 3) for k, ms in t.items()}
    out["saved_ms"] = round(out["legacy"]["median_ms"] - out["groups_image_frozen"]["median_ms"], 3)
    out["legacy_window_spread_ms"] = round(out["legacy"]["max_ms"] - out["legacy"]["min_ms"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--iters", type=int, default=400, help="calls per window of (a) and (b); (c) takes a tenth as many steps")
    a = ap.parse_args()
    m = _model()
    n = m.flat_buffers()[0].numel()
    res = {"shape": dict(S=S, T=T, A=A, V=V, B=B, dtype="fp32"),
           "method": f"HIP events, the two sides of a comparison alternating window by window in one process, median of {a.reps} "
                     f"windows of {a.iters} calls ((c): {max(a.iters // 10, 2)} steps), warm-up calls first"}
    res["a_one_segment_vs_vqa_adam"] = kernel_against_vqa_adam(n, a.reps, a.iters)
    res["b_step_without_image_vs_skip_path"] = step_without_image(m, a.reps, a.iters)
    res["c_feature_train_step"] = feature_train_step(m, a.reps, max(a.iters // 10, 2))
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
