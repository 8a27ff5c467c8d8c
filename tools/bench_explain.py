"""Gradient x input maps from cached features: what VqaNet.explain costs.

    python tools/bench_explain.py [--out-dir profiles] [--reps 7] [--iters 5]

North-star architecture, fp32, 224 x 224, T = 14, A = 1000; N = 256 images x 1 question and N = 32 x 8 (B = 256).  Per case,
in ONE process, interleaved windows timed with HIP events on the stream after a warm-up (the discipline of
tools/bench_multi_question.py; the figure is the median over --reps windows of --iters calls):

  answer / explain        on the same cache and questions: the difference is the price of the maps;
  explain_f16             the same call on the float16 cache;
  forward_backward        the only route to an explanation without explain: model(v[image_index]) with v.requires_grad, frozen
                          weights and a one-hot backward (every conv block forward and backward per pair; it yields d logit / d pixels, a
                          different and far more expensive quantity -- it is the cost a user pays today, not a parity check);
  attr_score / score      kernel 2 (ops.att_attr_score_grouped) against the grouped forward score kernel
                          (ops.att_score_grouped_fwd) on the same v', q', order and offsets: both stream the same v' tiles.

The driver never touches the GPU: the measurement is a child process under its own `timeout`, and a failure ends the run.
Output: one JSON object on stdout and in OUT_DIR/explain_bench.json.
"""
import json
import statistics

from bench_explain_common import A, S, SHAPES, T, V, main, setup, window as _window


def step_time(reps, iters):
    import torch
    from dl_vqa_amd import group_by_image, ops
    med = statistics.median
    res = {"shape": dict(S=S, T=T, A=A, V=V, dtype="fp32"),
           "method": f"HIP events, interleaved, median of {reps} windows of {iters} calls (kernels: {10 * iters}), 2 warm-up calls "
                     "per path; the forward+backward route's v[image_index] gather is outside its window", "cases": []}
    for N, per in SHAPES:
        cs = setup(N, per)
        m, B, v, q, ql, image_index, feats = cs.m, cs.B, cs.v, cs.q, cs.ql, cs.image_index, cs.feats
        for p in m.parameters():                         # a saliency user freezes the weights: only d logit / d v is computed
            p.requires_grad_(False)
        v_rep = v[image_index.cuda()].contiguous().requires_grad_(True)
        f16 = feats.to(torch.float16)
        cols = m.predict(feats, q, ql, image_index, k=1).indices[:, 0]
        onehot = torch.zeros(B, A, device="cuda").scatter_(1, cols[:, None], 1.0)

        def answer():
            return m.answer(feats, q, ql, image_index)

        def explain():
            return m.explain(feats, q, ql, image_index)

        def explain_f16():
            return m.explain(f16, q, ql, image_index)

        def forward_backward():
            v_rep.grad = None
            m(v_rep, q, ql).backward(onehot)

        # kernel 2 against the grouped forward score kernel, on the same operands
        eng, P = m._engine, m._param_dict()
        Pn, mid, G, mode = feats.vn.shape[1], eng.mid, eng.G, eng.att_mode
        order, offsets = (t.cuda() for t in group_by_image(image_index, N))
        wx, bx = P["attention.x_conv.weight"].view(G, -1), P["attention.x_conv.bias"]
        qp = torch.randn(B, mid, device="cuda")
        ds = torch.randn(B, G, Pn, device="cuda")
        r1 = torch.randn(B, Pn, device="cuda")
        out = torch.empty(B, Pn, device="cuda")

        def score():
            return ops.att_score_grouped_fwd(feats.vprime, qp, wx, bx, order, offsets, N, B, Pn, mode)

        def attr_score():
            return ops.att_attr_score_grouped(r1, ds, feats.vprime, qp, wx, order, offsets, N, B, Pn, mode, out=out)

        for _ in range(2):
            y_a, e = answer(), explain()
            explain_f16(), forward_backward(), score(), attr_score()
        torch.cuda.synchronize()
        same = bool(torch.equal(y_a, e.logits))
        t = {k: [] for k in ("answer", "explain", "explain_f16", "forward_backward", "score", "attr_score")}
        for _ in range(reps):
            t["answer"].append(_window(answer, iters))
            t["explain"].append(_window(explain, iters))
            t["explain_f16"].append(_window(explain_f16, iters))
            t["forward_backward"].append(_window(forward_backward, max(1, iters // 2)))
            t["score"].append(_window(score, 10 * iters))
            t["attr_score"].append(_window(attr_score, 10 * iters))
        ms = {k: med(x) for k, x in t.items()}
        tile_bytes = N * Pn * mid * 4
        case = dict(N=N, questions_per_image=per, B=B, P=Pn, mid=mid, G=G,
                    answer_ms=round(ms["answer"], 3), explain_ms=round(ms["explain"], 3),
                    maps_price_ms=round(ms["explain"] - ms["answer"], 3), explain_over_answer=round(ms["explain"] / ms["answer"], 3),
                    explain_f16_ms=round(ms["explain_f16"], 3), f16_over_fp32=round(ms["explain_f16"] / ms["explain"], 3),
                    forward_backward_ms=round(ms["forward_backward"], 3),
                    forward_backward_over_explain=round(ms["forward_backward"] / ms["explain"], 1),
                    score_kernel_us=round(1e3 * ms["score"], 1), attr_score_kernel_us=round(1e3 * ms["attr_score"], 1),
                    attr_over_score=round(ms["attr_score"] / ms["score"], 3),
                    vprime_bytes=tile_bytes, attr_score_vprime_TBps=round(tile_bytes / ms["attr_score"] / 1e9, 3),
                    min_max_ms={k: [round(min(x), 3), round(max(x), 3)] for k, x in t.items()},
                    explain_logits_equal_answer=same)
        res["cases"].append(case)
        del cs, m, v, v_rep, feats, f16
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main(__file__, step_time, "explain_bench.json", iters=5, limit=420)
