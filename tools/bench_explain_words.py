"""Per-token gradient x input from cached features: what VqaNet.explain_words costs.

    python tools/bench_explain_words.py [--out-dir profiles] [--reps 7] [--iters 5]

North-star architecture, 224 x 224, T = 14, A = 1000; N = 256 images x 1 question and N = 32 x 8 (B = 256); fp32 and float16
caches.  Per case, in ONE process, interleaved windows timed with HIP events on the stream after a warm-up (the discipline of
tools/bench_explain.py; the figure is the median over --reps windows of --iters calls):

  answer / explain / explain_words   on the same cache and questions: the differences are the price of the maps and of the words;
  dq / score_bwd                     kernel A (ops.att_attr_dq_grouped) against the kernel it derives from
                                     (ops.att_score_grouped_bwd at p = 0) on the same v', q', dscore, order and offsets, each with
                                     the bytes of the model below and the rate they give.  The training kernel has no float16
                                     form, so on a float16 cache kernel A stands alone;
  recurrence                         Engine._recurrence_bwd alone on the state one question front left, and its share of the call.

Byte model (compulsory traffic; the q' rows a workgroup re-reads per tile and wx come through L2 and are counted once):
  dq         reads v' [N*P, mid] (4 or 2 bytes), q' [B, mid], dscore [B, G, P], wx [G, mid]; writes dq_part [B*NT, mid]
  score_bwd  the same, plus writes dv' [N*P, mid] and dwx_part [N*NT, G, mid]
explain_words reads v' twice, once in explain's kernel 2 and once in kernel A: a fused walk would save at most kernel A's time,
which is reported next to the recurrence's.

The driver never touches the GPU: the measurement is a child process under its own `timeout`, and a failure ends the run.
Output: one JSON object on stdout and in OUT_DIR/explain_words_bench.json.
"""
import json
import statistics

from bench_explain_common import A, S, SHAPES, T, V, main, setup, window as _window


def dq_bytes(N, B, P, mid, G, NT, elt):
    return N * P * mid * elt + 4 * (B * mid + B * G * P + G * mid + B * NT * mid)


def score_bwd_bytes(N, B, P, mid, G, NT):
    return dq_bytes(N, B, P, mid, G, NT, 4) + 4 * (N * P * mid + N * NT * G * mid)


def step_time(reps, iters):
    import torch
    from dl_vqa_amd import group_by_image, ops
    med = statistics.median
    res = {"shape": dict(S=S, T=T, A=A, V=V),
           "method": f"HIP events, interleaved, median of {reps} windows of {iters} calls (kernels and the recurrence: {10 * iters}), "
                     "2 warm-up calls per path", "cases": []}
    for N, per in SHAPES:
        cs = setup(N, per)
        m, B, q, ql, image_index, f32 = cs.m, cs.B, cs.q, cs.ql, cs.image_index, cs.feats
        f16 = f32.to(torch.float16)
        eng, P = m._engine, m._param_dict()
        Pn, mid, G, mode, Q, H = f32.vn.shape[1], eng.mid, eng.G, eng.att_mode, eng.Q, eng.H
        order, offsets, img = (t.cuda() for t in (*group_by_image(image_index, N), image_index.to(torch.int32)))
        wx = P["attention.x_conv.weight"].view(G, -1)
        qp = torch.randn(B, mid, device="cuda")
        ds = torch.randn(B, G, Pn, device="cuda")
        NT = (Pn + 15) // 16
        part = torch.empty(B * NT, mid, device="cuda")
        # the recurrence alone: the state of one question front, d / d (question features) random
        with torch.cuda.device(f32.vn.device):
            txt, _ = eng._question_front(P, q, ql, f32.vn.device, 0.0, 0, None, side=False)
        dqf = torch.randn(B, Q, device="cuda")

        def recurrence():
            return eng._recurrence_bwd(P, txt.lstm, txt.q_len, dqf, Q, B, T)

        def score_bwd():
            return ops.att_score_grouped_bwd(ds, f32.vprime, qp, wx, order, offsets, N, B, Pn, mode, 0.0, 0)

        case = dict(N=N, questions_per_image=per, B=B, P=Pn, mid=mid, G=G, H=H, T=T, E=eng.E, caches={})
        for name, feats in (("fp32", f32), ("float16", f16)):
            elt = 4 if name == "fp32" else 2

            def answer():
                return m.answer(feats, q, ql, image_index)

            def explain():
                return m.explain(feats, q, ql, image_index)

            def words():
                return m.explain_words(feats, q, ql, image_index)

            def dq():
                return ops.att_attr_dq_grouped(ds, feats.vprime, qp, wx, order, offsets, N, B, Pn, mode, dq_part=part)

            fns = dict(answer=answer, explain=explain, explain_words=words, dq=dq, recurrence=recurrence)
            if name == "fp32":
                fns["score_bwd"] = score_bwd
            small = ("dq", "score_bwd", "recurrence")
            for _ in range(2):
                out = {k: f() for k, f in fns.items()}
            torch.cuda.synchronize()
            same = bool(torch.equal(out["explain_words"].maps, out["explain"].maps)
                        and torch.equal(out["explain_words"].logits, out["answer"]))
            if name == "fp32":
                same = same and bool(torch.equal(part, out["score_bwd"][1]))
            t = {k: [] for k in fns}
            for _ in range(reps):
                for k, f in fns.items():
                    t[k].append(_window(f, 10 * iters if k in small else iters))
            ms = {k: med(x) for k, x in t.items()}
            c = dict(answer_ms=round(ms["answer"], 3), explain_ms=round(ms["explain"], 3),
                     explain_words_ms=round(ms["explain_words"], 3),
                     words_price_over_explain_ms=round(ms["explain_words"] - ms["explain"], 3),
                     explain_words_over_answer=round(ms["explain_words"] / ms["answer"], 3),
                     dq_kernel_us=round(1e3 * ms["dq"], 1), dq_bytes=dq_bytes(N, B, Pn, mid, G, NT, elt),
                     dq_TBps=round(dq_bytes(N, B, Pn, mid, G, NT, elt) / ms["dq"] / 1e9, 3),
                     recurrence_ms=round(ms["recurrence"], 3), recurrence_share=round(ms["recurrence"] / ms["explain_words"], 3),
                     fused_walk_would_save_at_most_ms=round(ms["dq"], 3),
                     min_max_ms={k: [round(min(x), 4), round(max(x), 4)] for k, x in t.items()},
                     same_bits_as_explain_and_answer=same)
            if name == "fp32":
                c.update(score_bwd_kernel_us=round(1e3 * ms["score_bwd"], 1), score_bwd_bytes=score_bwd_bytes(N, B, Pn, mid, G, NT),
                         score_bwd_TBps=round(score_bwd_bytes(N, B, Pn, mid, G, NT) / ms["score_bwd"] / 1e9, 3),
                         dq_over_score_bwd=round(ms["dq"] / ms["score_bwd"], 3))
            case["caches"][name] = c
        res["cases"].append(case)
        del cs, m, f32, f16, txt
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main(__file__, step_time, "explain_words_bench.json", iters=5, limit=420)
