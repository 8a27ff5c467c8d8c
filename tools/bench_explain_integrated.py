"""Integrated gradients from cached features: what VqaNet.explain_integrated costs.

    python tools/bench_explain_integrated.py [--out-dir profiles] [--reps 7] [--iters 5]

North-star architecture, fp32, 224 x 224, T = 14, A = 1000; N = 256 images x 1 question and N = 32 x 8 (B = 256); steps = 16.
Per case, in ONE process, interleaved windows timed with HIP events on the stream after a warm-up (the discipline of
tools/bench_explain.py; the figure is the median over --reps windows of --iters calls):

  explain_integrated      the call itself, on the fp32 cache; explain_integrated_f16 on the float16 cache;
  composed                what a user can do without it: 16 explain() calls with the same columns on 16 caches scaled by alpha_s.
                          The scaled caches are built BEFORE the timed region (a user would pay for them too: 2 more passes over
                          vn and v' per step), and the host-side average of the 16 results is not timed either;
  explain / answer        the one-point rule and the base run, on the same cache and questions;
  path_score / path_attr  the two new kernels alone (ops.att_path_score_grouped, ops.att_path_attr_grouped, S = 16) next to score /
                          attr_score (ops.att_score_grouped_fwd, ops.att_attr_score_grouped) on the same v', q', order and
                          offsets: all four stream the same v' tiles once.

Acceptance: the slowest window of explain_integrated is below the fastest window of the composed route at both shapes
(`slowest_integrated_below_fastest_composed`).

The driver never touches the GPU: the measurement is a child process under its own `timeout`, and a failure ends the run.
Output: one JSON object on stdout and in OUT_DIR/explain_integrated_bench.json.
"""
import json
import statistics

from bench_explain_common import A, S, SHAPES, T, V, main, setup, window as _window

STEPS = 16


def step_time(reps, iters):
    import torch
    from dl_vqa_amd import ImageFeatures, group_by_image, ops
    from dl_vqa_amd.model import integrated_alphas
    med = statistics.median
    res = {"shape": dict(S=S, T=T, A=A, V=V, dtype="fp32", steps=STEPS),
           "method": f"HIP events, interleaved, median of {reps} windows of {iters} calls (kernels: {10 * iters}; composed: "
                     f"{max(1, iters // 2)} x {STEPS} explain calls), 2 warm-up calls per path; the composed route's scaled caches "
                     "are built outside its window", "cases": []}
    for N, per in SHAPES:
        cs = setup(N, per)
        m, B, q, ql, image_index, feats = cs.m, cs.B, cs.q, cs.ql, cs.image_index, cs.feats
        f16 = feats.to(torch.float16)
        cols = m.predict(feats, q, ql, image_index, k=1).indices[:, 0]
        alphas = integrated_alphas(STEPS)
        scaled = [ImageFeatures(feats.vn * a, feats.vprime * a, feats.grid, m) for a in alphas.tolist()]

        def answer():
            return m.answer(feats, q, ql, image_index)

        def explain():
            return m.explain(feats, q, ql, image_index)

        def integrated():
            return m.explain_integrated(feats, q, ql, image_index, steps=STEPS)

        def integrated_f16():
            return m.explain_integrated(f16, q, ql, image_index, steps=STEPS)

        def composed():
            return [m.explain(sc, q, ql, image_index, answers=cols) for sc in scaled]

        # the two new kernels against the kernels they extend, on the same operands
        eng, P = m._engine, m._param_dict()
        Pn, mid, G, mode = feats.vn.shape[1], eng.mid, eng.G, eng.att_mode
        order, offsets = (t.cuda() for t in group_by_image(image_index, N))
        wx, bx = P["attention.x_conv.weight"].view(G, -1), P["attention.x_conv.bias"]
        al = alphas.cuda()
        qp = torch.randn(B, mid, device="cuda")
        ds, r1 = torch.randn(B, G, Pn, device="cuda"), torch.randn(B, Pn, device="cuda")
        ds_s, r1_s = torch.randn(B, STEPS, G, Pn, device="cuda"), torch.randn(B, STEPS, Pn, device="cuda")
        out, out_s = torch.empty(B, Pn, device="cuda"), torch.empty(B, STEPS, G, Pn, device="cuda")

        def score():
            return ops.att_score_grouped_fwd(feats.vprime, qp, wx, bx, order, offsets, N, B, Pn, mode)

        def attr_score():
            return ops.att_attr_score_grouped(r1, ds, feats.vprime, qp, wx, order, offsets, N, B, Pn, mode, out=out)

        def path_score():
            return ops.att_path_score_grouped(feats.vprime, qp, wx, bx, al, order, offsets, N, B, Pn, mode, out=out_s)

        def path_attr():
            return ops.att_path_attr_grouped(r1_s, ds_s, feats.vprime, qp, wx, al, 1.0 / STEPS, order, offsets, N, B, Pn, mode,
                                             out=out)

        for _ in range(2):
            y_a, e, ig = answer(), explain(), integrated()
            integrated_f16(), composed(), score(), attr_score(), path_score(), path_attr()
        torch.cuda.synchronize()
        same = bool(torch.equal(y_a, ig.logits)) and bool(torch.equal(e.answers, ig.answers))
        gap = float(ig.completeness_gap().abs().max())
        names = ("answer", "explain", "integrated", "integrated_f16", "composed", "score", "attr_score", "path_score", "path_attr")
        t = {k: [] for k in names}
        for _ in range(reps):
            t["answer"].append(_window(answer, iters))
            t["explain"].append(_window(explain, iters))
            t["integrated"].append(_window(integrated, iters))
            t["integrated_f16"].append(_window(integrated_f16, iters))
            t["composed"].append(_window(composed, max(1, iters // 2)))
            for k, fn in (("score", score), ("attr_score", attr_score), ("path_score", path_score), ("path_attr", path_attr)):
                t[k].append(_window(fn, 10 * iters))
        ms = {k: med(x) for k, x in t.items()}
        tile_bytes = N * Pn * mid * 4
        case = dict(N=N, questions_per_image=per, B=B, P=Pn, mid=mid, G=G, steps=STEPS,
                    explain_integrated_ms=round(ms["integrated"], 3), explain_integrated_f16_ms=round(ms["integrated_f16"], 3),
                    composed_ms=round(ms["composed"], 3), composed_over_integrated=round(ms["composed"] / ms["integrated"], 2),
                    explain_ms=round(ms["explain"], 3), answer_ms=round(ms["answer"], 3),
                    integrated_over_explain=round(ms["integrated"] / ms["explain"], 2),
                    slowest_integrated_below_fastest_composed=bool(max(t["integrated"]) < min(t["composed"])),
                    score_kernel_us=round(1e3 * ms["score"], 1), path_score_kernel_us=round(1e3 * ms["path_score"], 1),
                    attr_score_kernel_us=round(1e3 * ms["attr_score"], 1), path_attr_kernel_us=round(1e3 * ms["path_attr"], 1),
                    # the bytes model of the two walks: v' once each, whatever the steps; the composed route reads it 2 * steps times
                    vprime_bytes=tile_bytes, walks_vprime_bytes=2 * tile_bytes, composed_vprime_bytes=2 * STEPS * tile_bytes,
                    path_score_written_bytes=B * STEPS * G * Pn * 4, path_attr_read_bytes=B * STEPS * (G + 1) * Pn * 4,
                    min_max_ms={k: [round(min(x), 3), round(max(x), 3)] for k, x in t.items()},
                    logits_and_answers_equal=same, completeness_gap_max=gap)
        res["cases"].append(case)
        del cs, m, feats, f16, scaled
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main(__file__, step_time, "explain_integrated_bench.json", iters=5, limit=420)
