"""Deletion and insertion curves from cached features: what VqaNet.explain_faithfulness costs.

    python tools/bench_explain_faithfulness.py [--out-dir profiles] [--reps 7] [--iters 3]

North-star architecture, 224 x 224, T = 14, A = 1000; N = 256 images x 1 question and N = 32 x 8 (B = 256), fp32 and float16
caches.  Per case, in ONE process, interleaved windows timed with HIP events on the stream after a warm-up (the discipline of
tools/bench_explain.py; the figure is the median over --reps windows of --iters calls):

  answer / occlusion_w1     on the same cache and questions: what the curves are compared with;
  faithfulness / _f16       explain_faithfulness with a random map on the device; _f16: the same call on the float16 cache;
  brute_force (SCALED)      the only route to the same numbers without this call: answer() on a bank that holds one copy of its
                            image per question with the absent rows zeroed, once per step of each curve.  Eight set sizes are
                            timed and the figure is SCALED by 2 (P + 1) / 8 -- nobody runs 1354 answer() calls to find this out;
  kernel_curves / _w1       vqa_occl_curves (its three launches) and vqa_occl_logit window 1 alone on the same U (of every asked
                            image in one buffer), and vqa_rank_desc alone.  Byte model: one reading of U is B * P * G * hid * 4
                            bytes; vqa_occl_logit makes one, vqa_occl_curves makes THREE (the chunk sums, the insertion walk, the
                            deletion walk; the chunk sums, prefixes and suffixes add 7 / L of a reading), so its rate is stated
                            for three readings.

The driver never touches the GPU: the measurement is a child process under its own `timeout`, and a failure ends the run.
Output: one JSON object on stdout and in OUT_DIR/explain_faithfulness_bench.json.
"""
import json
import statistics

from bench_explain_common import A, S, SHAPES, T, V, main, setup, window as _window

BRUTE_SIZES = 8
U_READINGS = 3


def step_time(reps, iters):
    import torch
    from dl_vqa_amd import ImageFeatures, compact_image_index, ops
    med = statistics.median
    res = {"shape": dict(S=S, T=T, A=A, V=V, dtype="fp32"),
           "method": f"HIP events, interleaved, median of {reps} windows of {iters} calls (kernels: {10 * iters}), 2 warm-up calls "
                     f"per path; brute_force: answer() on {BRUTE_SIZES} zeroed per-question banks, SCALED by 2 (P + 1) / "
                     f"{BRUTE_SIZES}; no hardware counters were collected",
           "cases": []}
    for N, per in SHAPES:
        cs = setup(N, per)
        m, B, q, ql, image_index, feats = cs.m, cs.B, cs.q, cs.ql, cs.image_index, cs.feats
        f16 = feats.to(torch.float16)
        del cs
        Pn = feats.vn.shape[1]
        dev = feats.vn.device
        maps = torch.randn(B, Pn, device=dev)
        order = ops.rank_desc(maps).long()
        # the brute-force route: per-question banks with the first k positions of each question's ranking zeroed
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

        def occlusion():
            return m.explain_occlusion(feats, q, ql, image_index)

        def brute():
            for z in zeroed:
                m.answer(z, q, ql, each)

        def faithfulness():
            return m.explain_faithfulness(feats, q, ql, image_index, maps)

        def faithfulness_f16():
            return m.explain_faithfulness(f16, q, ql, image_index, maps)

        # the kernels alone, on operands of the call's shapes: U of every asked image in one buffer
        eng, P = m._engine, m._param_dict()
        G, hid, gh, gw = eng.G, eng.hid, *feats.grid
        rows, slot, _, _ = compact_image_index(image_index, N)
        slot = slot.to(dev)
        score = 2 * torch.randn(B, G, Pn, device=dev)
        probs = torch.softmax(score, -1)
        U = torch.randn(rows.numel(), Pn, G, hid, device=dev)
        Z = torch.randn(B, G, hid, device=dev)
        base = torch.randn(B, hid, device=dev)
        cnull = score.mean(-1).contiguous()
        logits = torch.randn(B, A, device=dev)
        cols = torch.randint(0, A, (B,), dtype=torch.int32, device=dev)
        out1 = torch.empty(B, Pn, device=dev)
        out2 = (torch.empty(B, Pn + 1, device=dev), torch.empty(B, Pn + 1, device=dev))
        order32 = torch.empty(B, Pn, dtype=torch.int32, device=dev)
        ws = ops.occl_curves_workspace(B, Pn, G, hid, dev)
        w2, b2 = P["classifier.lin2.weight"], P["classifier.lin2.bias"]

        def kernel_rank():
            return ops.rank_desc(maps, out=order32)

        def kernel_curves():
            return ops.occl_curves(base, U, slot, probs, score, cnull, w2, b2, cols, order32, out=out2, workspace=ws)

        def kernel_w1():
            return ops.occl_logit(base, Z, U, slot, probs, score, cnull, w2, b2, cols, logits, gh, gw, 1, out=out1)

        kernel_rank()
        paths = {"answer": (answer, iters), "occlusion_w1": (occlusion, iters), "faithfulness": (faithfulness, iters),
                 "faithfulness_f16": (faithfulness_f16, iters), "brute_force": (brute, 1), "kernel_rank": (kernel_rank, 10 * iters),
                 "kernel_curves": (kernel_curves, 10 * iters), "kernel_w1": (kernel_w1, 10 * iters)}
        for _ in range(2):
            for fn, _n in paths.values():
                fn()
        torch.cuda.synchronize()
        same = bool(torch.equal(answer(), faithfulness().logits))
        t = {k: [] for k in paths}
        for _ in range(reps):
            for k, (fn, n) in paths.items():
                t[k].append(_window(fn, n))
        ms = {k: med(x) for k, x in t.items()}
        brute_ms = ms["brute_force"] * 2 * (Pn + 1) / BRUTE_SIZES
        u_bytes = B * Pn * G * hid * 4
        case = dict(N=N, questions_per_image=per, B=B, P=Pn, G=G, hid=hid, chunk_steps=ops.occl_curves_chunk(),
                    **{k + "_ms": round(x, 3) for k, x in ms.items() if k != "brute_force" and not k.startswith("kernel")},
                    brute_force_scaled_ms=round(brute_ms, 1), brute_force_set_sizes_timed=BRUTE_SIZES,
                    brute_force_over_faithfulness=round(brute_ms / ms["faithfulness"], 1),
                    faithfulness_over_answer=round(ms["faithfulness"] / ms["answer"], 2),
                    faithfulness_over_occlusion_w1=round(ms["faithfulness"] / ms["occlusion_w1"], 2),
                    f16_over_fp32=round(ms["faithfulness_f16"] / ms["faithfulness"], 3),
                    kernel_rank_us=round(1e3 * ms["kernel_rank"], 1), kernel_curves_us=round(1e3 * ms["kernel_curves"], 1),
                    kernel_w1_us=round(1e3 * ms["kernel_w1"], 1),
                    kernel_curves_over_w1=round(ms["kernel_curves"] / ms["kernel_w1"], 2),
                    U_bytes_per_reading=u_bytes, curves_U_readings=U_READINGS,
                    kernel_curves_TBps_of_three_readings=round(U_READINGS * u_bytes / ms["kernel_curves"] / 1e9, 3),
                    kernel_w1_TBps=round(u_bytes / ms["kernel_w1"] / 1e9, 3),
                    workspace_bytes=ws.numel() * 4,
                    min_max_ms={k: [round(min(x), 3), round(max(x), 3)] for k, x in t.items()},
                    faithfulness_logits_equal_answer=same)
        res["cases"].append(case)
        del m, feats, f16, zeroed, U, ws
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main(__file__, step_time, "explain_faithfulness_bench.json", iters=3, limit=540)
