"""Probability curves and flip points from cached features: what VqaNet.explain_faithfulness_probs costs.

    python tools/bench_explain_prob_curves.py [--out-dir profiles] [--reps 7] [--iters 3]

North-star architecture, 224 x 224, T = 14, A = 1000; N = 256 images x 1 question and N = 32 x 8 (B = 256), fp32 caches.  Per
case, in ONE process, interleaved windows timed with HIP events on the stream after a warm-up (the discipline of
tools/bench_explain.py; the figure is the median over --reps windows of --iters calls):

  answer / faithfulness     on the same cache and questions: what the probability curves are compared with (faithfulness is also
                            compared with the parent commit's profiles/explain_faithfulness_bench.json);
  prob_curves               explain_faithfulness_probs with a random map on the device;
  brute_force (SCALED)      the only route to the same numbers without this call: answer() on a bank that holds one copy of its
                            image per question with the absent rows zeroed, then torch.softmax and arg-max, once per step of each
                            curve.  Eight set sizes are timed and the figure is SCALED by 2 (P + 1) / 8;
  kernel_hidden / _curves   vqa_occl_curves_hidden and vqa_occl_curves (three launches each) alone on the same U (of every asked
                            image in one buffer).  Byte model: both make THREE readings of U (B * P * G * hid * 4 bytes each);
                            the hidden walk also writes H, 2 (P + 1) * hid * 4 bytes per question;
  copy                      a device-to-device copy of H's size: the rate at which that extra traffic is charged;
  gemm                      ops.gemm(H, lin2.weight, bias1 = lin2.bias) alone at the sub-chunk's shape, 2 * rows * A * hid FLOP;
  kernel_pick / _topk1      vqa_softmax_pick and vqa_softmax_topk(k = 1) alone on the sub-chunk's logits.

The driver never touches the GPU: the measurement is a child process under its own `timeout`, and a failure ends the run.
Output: one JSON object on stdout and in OUT_DIR/explain_prob_curves_bench.json.
"""
import json
import os
import statistics

from bench_explain_common import A, ROOT, S, SHAPES, T, V, main, setup, window as _window

BRUTE_SIZES = 8
U_READINGS = 3


def _parent_faithfulness():
    """{(N, per): (median, min, max) ms} of explain_faithfulness as the parent commit recorded it."""
    try:
        cases = json.load(open(os.path.join(ROOT, "profiles", "explain_faithfulness_bench.json")))["cases"]
    except (OSError, ValueError, KeyError):
        return {}
    return {(c["N"], c["questions_per_image"]): (c["faithfulness_ms"], *c["min_max_ms"]["faithfulness"]) for c in cases}


def step_time(reps, iters):
    import torch
    from dl_vqa_amd import ImageFeatures, compact_image_index, ops
    med = statistics.median
    parent = _parent_faithfulness()
    res = {"shape": dict(S=S, T=T, A=A, V=V, dtype="fp32"),
           "method": f"HIP events, interleaved, median of {reps} windows of {iters} calls (kernels: {10 * iters}), 2 warm-up calls "
                     f"per path; brute_force: answer() + torch.softmax + arg-max on {BRUTE_SIZES} zeroed per-question banks, SCALED "
                     f"by 2 (P + 1) / {BRUTE_SIZES}; no hardware counters were collected",
           "cases": []}
    for N, per in SHAPES:
        cs = setup(N, per)
        m, B, q, ql, image_index, feats = cs.m, cs.B, cs.q, cs.ql, cs.image_index, cs.feats
        del cs
        Pn = feats.vn.shape[1]
        dev = feats.vn.device
        maps = torch.randn(B, Pn, device=dev)
        order = ops.rank_desc(maps).long()
        pick = image_index.to(dev)
        each = list(range(B))
        zeroed = []
        for k in [round(i * Pn / (BRUTE_SIZES - 1)) for i in range(BRUTE_SIZES)]:
            keep = torch.ones(B, Pn, device=dev)
            keep.scatter_(1, order[:, :k], 0.0)
            vn = (feats.vn[pick] * keep[..., None]).contiguous()
            vp = (feats.vprime.view(N, Pn, -1)[pick] * keep[..., None]).reshape(B * Pn, -1).contiguous()
            zeroed.append(ImageFeatures(vn, vp, feats.grid, m))

        def answer():
            return m.answer(feats, q, ql, image_index)

        def faithfulness():
            return m.explain_faithfulness(feats, q, ql, image_index, maps)

        def prob_curves():
            return m.explain_faithfulness_probs(feats, q, ql, image_index, maps)

        def brute():
            for z in zeroed:
                p = torch.softmax(m.answer(z, q, ql, each), -1)
                p.max(-1)

        # the kernels alone, on operands of the call's shapes: U of every asked image in one buffer
        eng, P = m._engine, m._param_dict()
        G, hid = eng.G, eng.hid
        rows, slot, _, _ = compact_image_index(image_index, N)
        slot = slot.to(dev)
        score = 2 * torch.randn(B, G, Pn, device=dev)
        probs = torch.softmax(score, -1)
        U = torch.randn(rows.numel(), Pn, G, hid, device=dev)
        base = torch.randn(B, hid, device=dev)
        cnull = score.mean(-1).contiguous()
        cols = torch.randint(0, A, (B,), dtype=torch.int32, device=dev)
        out2 = (torch.empty(B, Pn + 1, device=dev), torch.empty(B, Pn + 1, device=dev))
        order32 = ops.rank_desc(maps)
        ws = ops.occl_curves_workspace(B, Pn, G, hid, dev)
        w2, b2 = P["classifier.lin2.weight"], P["classifier.lin2.bias"]
        H = torch.empty(B, 2, Pn + 1, hid, device=dev)
        H2 = torch.empty_like(H)
        K = 2 * (Pn + 1)
        sub = min(B, eng.prob_curve_questions(Pn))
        Y = torch.empty(sub * K, A, device=dev)
        pick_out = (torch.empty(sub * K, dtype=torch.int32, device=dev), torch.empty(sub * K, device=dev),
                    torch.empty(sub * K, device=dev))

        def kernel_curves():
            return ops.occl_curves(base, U, slot, probs, score, cnull, w2, b2, cols, order32, out=out2, workspace=ws)

        def kernel_hidden():
            return ops.occl_curves_hidden(base, U, slot, probs, score, cnull, order32, out=H, workspace=ws)

        def copy():
            return H2.copy_(H)

        def gemm():
            return ops.gemm(H[:sub].view(sub * K, hid), w2, Y, sub * K, A, hid, bias1=b2)

        def kernel_pick():
            return ops.softmax_pick(Y, cols[:sub], K, out=pick_out)

        def kernel_topk1():
            return ops.softmax_topk(Y, 1)

        paths = {"answer": (answer, iters), "faithfulness": (faithfulness, iters), "prob_curves": (prob_curves, iters),
                 "brute_force": (brute, 1), "kernel_curves": (kernel_curves, 10 * iters), "kernel_hidden": (kernel_hidden, 10 * iters),
                 "copy": (copy, 10 * iters), "gemm": (gemm, iters), "kernel_pick": (kernel_pick, 10 * iters),
                 "kernel_topk1": (kernel_topk1, 10 * iters)}
        for _ in range(2):
            for fn, _n in paths.values():
                fn()
        torch.cuda.synchronize()
        got, ref = prob_curves(), faithfulness()
        same = bool(torch.equal(answer(), got.logits) and torch.equal(got.order, ref.order))
        t = {k: [] for k in paths}
        for _ in range(reps):
            for k, (fn, n) in paths.items():
                t[k].append(_window(fn, n))
        ms = {k: med(x) for k, x in t.items()}
        brute_ms = ms["brute_force"] * K / BRUTE_SIZES
        u_bytes, h_bytes = B * Pn * G * hid * 4, B * K * hid * 4
        copy_rate = 2 * h_bytes / ms["copy"] / 1e9                    # TB/s, a read and a write per byte
        extra_ms = h_bytes / (copy_rate * 1e9)                        # what writing H costs at that rate
        flop = 2.0 * sub * K * A * hid
        was = parent.get((N, per))
        case = dict(N=N, questions_per_image=per, B=B, P=Pn, G=G, hid=hid, A=A, chunk_steps=ops.occl_curves_chunk(),
                    sub_chunk_questions=sub, sub_chunks=-(-B // sub), sub_chunk_rows=sub * K,
                    **{k + "_ms": round(ms[k], 3) for k in ("answer", "faithfulness", "prob_curves", "gemm")},
                    brute_force_scaled_ms=round(brute_ms, 1), brute_force_set_sizes_timed=BRUTE_SIZES,
                    brute_force_over_prob_curves=round(brute_ms / ms["prob_curves"], 1),
                    prob_curves_over_faithfulness=round(ms["prob_curves"] / ms["faithfulness"], 2),
                    prob_curves_over_answer=round(ms["prob_curves"] / ms["answer"], 2),
                    kernel_curves_us=round(1e3 * ms["kernel_curves"], 1), kernel_hidden_us=round(1e3 * ms["kernel_hidden"], 1),
                    kernel_hidden_over_curves=round(ms["kernel_hidden"] / ms["kernel_curves"], 2),
                    U_bytes_per_reading=u_bytes, U_readings=U_READINGS, H_bytes=h_bytes,
                    copy_TBps=round(copy_rate, 3), H_write_at_copy_rate_us=round(1e3 * extra_ms, 1),
                    kernel_hidden_minus_curves_us=round(1e3 * (ms["kernel_hidden"] - ms["kernel_curves"]), 1),
                    kernel_hidden_TBps_of_three_readings_and_H=round((U_READINGS * u_bytes + h_bytes) / ms["kernel_hidden"] / 1e9, 3),
                    gemm_flop=flop, gemm_TFLOPs=round(flop / ms["gemm"] / 1e9, 1),
                    gemm_all_sub_chunks_ms=round(ms["gemm"] * B / sub, 3),
                    kernel_pick_us=round(1e3 * ms["kernel_pick"], 1), kernel_topk1_us=round(1e3 * ms["kernel_topk1"], 1),
                    kernel_pick_over_topk1=round(ms["kernel_pick"] / ms["kernel_topk1"], 2),
                    logits_bytes_per_sub_chunk=sub * K * A * 4,
                    kernel_pick_TBps=round(sub * K * A * 4 / ms["kernel_pick"] / 1e9, 3),
                    faithfulness_parent_ms=None if was is None else was[0],
                    faithfulness_parent_min_max_ms=None if was is None else list(was[1:]),
                    faithfulness_outside_parent_spread=None if was is None else not (was[1] <= ms["faithfulness"] <= was[2]),
                    min_max_ms={k: [round(min(x), 3), round(max(x), 3)] for k, x in t.items()},
                    logits_equal_answer_and_order_equal_faithfulness=same)
        res["cases"].append(case)
        del m, feats, zeroed, U, ws, H, H2, Y
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main(__file__, step_time, "explain_prob_curves_bench.json", iters=3, limit=540)
