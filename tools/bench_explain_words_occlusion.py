"""Exact word occlusion from cached features: what VqaNet.explain_words_occlusion costs.

    python tools/bench_explain_words_occlusion.py [--out-dir profiles] [--reps 7] [--iters 3]

North-star architecture, fp32, 224 x 224, T = 14, A = 1000; 256 questions on 256 images and on 32 images x 8 questions.  Lengths:
the fixed ragged pattern LENGTHS repeated over the batch (mean 7.0, 2 .. 14).  Per case, in ONE process, interleaved windows
timed with HIP events on the stream after a warm-up (the discipline of tools/bench_explain_occlusion.py; the figure is the
median over --reps windows of --iters calls, and min .. max over the windows is reported beside it):

  answer / explain_words    on the same cache and questions: what the call is compared with;
  words_occlusion           the new call: answer's front and tail, the variant chains from the saved base states, the variant
                            tail;
  brute_force               the only route to the same numbers without this call, from the public API: answer() for the base
                            logits, encode_questions on the V = sum_b q_len[b] questions with the padding token substituted for
                            one word (the whole recurrence for every variant, 2 * T steps per variant row), answer_pairs on them.
                            The substituted questions are built once, outside the timed windows -- in the route's favour.

It also reports V, the recurrent row-steps of both routes and the largest difference between their words.

The driver never touches the GPU: the measurement is a child process under its own `timeout`, and a failure ends the run.
Output: one JSON object on stdout and in OUT_DIR/explain_words_occlusion_bench.json.
"""
import json
import statistics

from bench_explain_common import A, S, SHAPES, T, V, main, setup, window as _window

LENGTHS = (3, 5, 7, 9, 11, 14, 4, 6, 8, 10, 2, 5, 7, 9, 6, 6)      # mean 7.0


def step_time(reps, iters):
    import torch
    from dl_vqa_amd.model import word_occlusion_table
    med = statistics.median
    res = {"shape": dict(S=S, T=T, A=A, V=V, dtype="fp32", lengths=list(LENGTHS), mean_length=sum(LENGTHS) / len(LENGTHS)),
           "method": f"HIP events, interleaved, median of {reps} windows of {iters} calls, 2 warm-up calls per path; brute_force: "
                     "answer + encode_questions on the substituted questions (built outside the windows) + answer_pairs",
           "cases": []}
    for N, per in SHAPES:
        cs = setup(N, per, questions_on_device=False)
        m, B, q, image_index, feats = cs.m, cs.B, cs.q, cs.image_index, cs.feats
        del cs
        assert float(m.text.embedding.weight[0].detach().abs().max()) == 0.0      # the brute-force route needs a zero padding row
        ql = torch.tensor([LENGTHS[b % len(LENGTHS)] for b in range(B)])
        q = torch.where(torch.arange(T)[None, :] < ql[:, None], q.clamp(min=1), torch.zeros_like(q))
        tab = word_occlusion_table(ql, T)
        vb, vt = tab.fwd_b.long(), tab.fwd_t.long()
        q_sub = q[vb].clone()
        q_sub[torch.arange(tab.V), vt] = 0
        q, ql_dev, q_sub, ql_sub, img_sub = q.cuda(), ql.cuda(), q_sub.cuda(), ql[vb].cuda(), image_index[vb]
        pair_rows = torch.arange(tab.V)

        def answer():
            return m.answer(feats, q, ql_dev, image_index)

        def explain_words():
            return m.explain_words(feats, q, ql_dev, image_index)

        def words_occlusion():
            return m.explain_words_occlusion(feats, q, ql_dev, image_index)

        def brute():
            base = m.answer(feats, q, ql_dev, image_index)
            return base, m.answer_pairs(feats, m.encode_questions(q_sub, ql_sub), img_sub, pair_rows)

        paths = {"answer": answer, "explain_words": explain_words, "words_occlusion": words_occlusion, "brute_force": brute}
        for _ in range(2):
            for fn in paths.values():
                fn()
        torch.cuda.synchronize()
        got = words_occlusion()
        base, occluded = brute()
        cols = got.answers
        route = torch.zeros(B, T, device=q.device)
        route[vb.cuda(), vt.cuda()] = (base.gather(1, cols[:, None])[:, 0][vb.cuda()]
                                       - occluded.gather(1, cols[vb.cuda()][:, None])[:, 0])
        diff = float((got.words - route).abs().max())
        t = {k: [] for k in paths}
        for _ in range(reps):
            for k, fn in paths.items():
                t[k].append(_window(fn, iters))
        ms = {k: med(x) for k, x in t.items()}
        case = dict(N=N, questions_per_image=per, B=B, P=feats.vn.shape[1], variants=tab.V,
                    row_steps_words_occlusion=tab.row_steps, row_steps_brute_force=2 * T * tab.V,
                    row_steps_ratio=round(tab.row_steps / (2 * T * tab.V), 3),
                    **{k + "_ms": round(x, 3) for k, x in ms.items()},
                    min_max_ms={k: [round(min(x), 3), round(max(x), 3)] for k, x in t.items()},
                    brute_force_over_words_occlusion=round(ms["brute_force"] / ms["words_occlusion"], 2),
                    slowest_words_occlusion_window_below_fastest_brute_force=bool(max(t["words_occlusion"]) < min(t["brute_force"])),
                    words_occlusion_over_answer=round(ms["words_occlusion"] / ms["answer"], 2),
                    words_occlusion_over_explain_words=round(ms["words_occlusion"] / ms["explain_words"], 2),
                    max_abs_words=round(float(got.words.abs().max()), 6), max_abs_diff_from_brute_force=diff,
                    logits_equal_answer=bool(torch.equal(got.logits, base)))
        res["cases"].append(case)
        del m, feats
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main(__file__, step_time, "explain_words_occlusion_bench.json", iters=3, limit=540)
