"""Occlusion maps from cached features: what VqaNet.explain_occlusion costs.

    python tools/bench_explain_occlusion.py [--out-dir profiles] [--reps 7] [--iters 3]

North-star architecture, fp32, 224 x 224, T = 14, A = 1000; N = 256 images x 1 question and N = 32 x 8 (B = 256).  Per case,
in ONE process, interleaved windows timed with HIP events on the stream after a warm-up (the discipline of
tools/bench_explain.py; the figure is the median over --reps windows of --iters calls):

  answer / explain          on the same cache and questions: what the occlusion maps are compared with;
  occlusion_w1 / _w3        explain_occlusion with window 1 and 3; _f16: the same calls on the float16 cache;
  brute_force (SCALED)      the only route to the same numbers without this call: answer() on a cache with one position's rows
                            zeroed, once per position.  Eight positions are timed and the figure is SCALED by P / 8 -- nobody
                            runs 677 answer() calls to find this out;
  kernel_w1 / _w3           vqa_occl_logit alone on the call's own operands (U of every asked image in one buffer), with its
                            bandwidth under its own byte model: U read once per question (B * P * G * hid * 4 bytes; a larger
                            window re-reads rows its neighbours have just read, from the cache), the rest small.

The driver never touches the GPU: the measurement is a child process under its own `timeout`, and a failure ends the run.
Output: one JSON object on stdout and in OUT_DIR/explain_occlusion_bench.json.
"""
import json
import statistics

from bench_explain_common import A, S, SHAPES, T, V, main, setup, window as _window

BRUTE_POSITIONS = 8


def step_time(reps, iters):
    import torch
    from dl_vqa_amd import ImageFeatures, compact_image_index, ops
    med = statistics.median
    res = {"shape": dict(S=S, T=T, A=A, V=V, dtype="fp32"),
           "method": f"HIP events, interleaved, median of {reps} windows of {iters} calls (kernels: {10 * iters}), 2 warm-up calls "
                     f"per path; brute_force: answer() on {BRUTE_POSITIONS} zeroed caches, SCALED by P / {BRUTE_POSITIONS}",
           "cases": []}
    for N, per in SHAPES:
        cs = setup(N, per)
        m, B, q, ql, image_index, feats = cs.m, cs.B, cs.q, cs.ql, cs.image_index, cs.feats
        f16 = feats.to(torch.float16)
        del cs
        Pn = feats.vn.shape[1]
        zeroed = []
        for p in range(0, Pn, Pn // BRUTE_POSITIONS)[:BRUTE_POSITIONS]:
            vn, vp = feats.vn.clone(), feats.vprime.clone()
            vn[:, p, :] = 0
            vp.view(N, Pn, -1)[:, p, :] = 0
            zeroed.append(ImageFeatures(vn, vp, feats.grid, m))

        def answer():
            return m.answer(feats, q, ql, image_index)

        def explain():
            return m.explain(feats, q, ql, image_index)

        def brute():
            for z in zeroed:
                m.answer(z, q, ql, image_index)

        occl = {f"occlusion_w{w}{sfx}": (lambda w=w, c=c: m.explain_occlusion(c, q, ql, image_index, window=w))
                for w in (1, 3) for sfx, c in (("", feats), ("_f16", f16))}

        # the kernel alone, on operands of the call's shapes: U of every asked image in one buffer
        eng, P = m._engine, m._param_dict()
        G, hid, gh, gw = eng.G, eng.hid, *feats.grid
        dev = feats.vn.device
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
        out = torch.empty(B, Pn, device=dev)
        kern = {f"kernel_w{w}": (lambda w=w: ops.occl_logit(base, Z, U, slot, probs, score, cnull, P["classifier.lin2.weight"],
                                                            P["classifier.lin2.bias"], cols, logits, gh, gw, w, out=out))
                for w in (1, 3)}

        paths = {"answer": (answer, iters), "explain": (explain, iters), **{k: (f, iters) for k, f in occl.items()},
                 "brute_force": (brute, 1), **{k: (f, 10 * iters) for k, f in kern.items()}}
        for _ in range(2):
            for fn, _n in paths.values():
                fn()
        torch.cuda.synchronize()
        o = occl["occlusion_w1"]()
        same = bool(torch.equal(answer(), o.logits))
        t = {k: [] for k in paths}
        for _ in range(reps):
            for k, (fn, n) in paths.items():
                t[k].append(_window(fn, n))
        ms = {k: med(x) for k, x in t.items()}
        brute_ms = ms["brute_force"] * Pn / BRUTE_POSITIONS
        u_bytes = B * Pn * G * hid * 4
        case = dict(N=N, questions_per_image=per, B=B, P=Pn, G=G, hid=hid,
                    **{k + "_ms": round(x, 3) for k, x in ms.items() if k != "brute_force" and not k.startswith("kernel")},
                    brute_force_scaled_ms=round(brute_ms, 1), brute_force_positions_timed=BRUTE_POSITIONS,
                    brute_force_over_occlusion_w1=round(brute_ms / ms["occlusion_w1"], 1),
                    occlusion_w1_over_answer=round(ms["occlusion_w1"] / ms["answer"], 2),
                    occlusion_w1_over_explain=round(ms["occlusion_w1"] / ms["explain"], 2),
                    occlusion_w3_over_w1=round(ms["occlusion_w3"] / ms["occlusion_w1"], 3),
                    f16_over_fp32_w1=round(ms["occlusion_w1_f16"] / ms["occlusion_w1"], 3),
                    kernel_w1_us=round(1e3 * ms["kernel_w1"], 1), kernel_w3_us=round(1e3 * ms["kernel_w3"], 1),
                    kernel_U_bytes=u_bytes, kernel_w1_TBps=round(u_bytes / ms["kernel_w1"] / 1e9, 3),
                    kernel_w3_TBps_of_distinct_bytes=round(u_bytes / ms["kernel_w3"] / 1e9, 3),
                    U_gemm_gflop=round(2 * rows.numel() * Pn * G * hid * eng.C / 1e9, 1),
                    min_max_ms={k: [round(min(x), 3), round(max(x), 3)] for k, x in t.items()},
                    occlusion_logits_equal_answer=same)
        res["cases"].append(case)
        del m, feats, f16, zeroed, U
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main(__file__, step_time, "explain_occlusion_bench.json", iters=3, limit=540)
