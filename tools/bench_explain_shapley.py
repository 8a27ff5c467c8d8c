"""Sampled Shapley maps from cached features: what VqaNet.explain_shapley costs.

    python tools/bench_explain_shapley.py [--out-dir profiles] [--reps 7] [--iters 3]

North-star architecture, 224 x 224, T = 14, A = 1000; N = 256 images x 1 question and N = 32 x 8 (B = 256), permutations = 16
(8 drawn orders, each walked with its reverse).  Per case, in ONE process, interleaved windows timed with HIP events on the
stream after a warm-up (the discipline of tools/bench_explain.py; the figure is the median over --reps windows of --iters
calls, with min..max beside it):

  answer / occlusion_w1     on the same cache and questions: what the call is compared with;
  shapley                   explain_shapley(permutations=16) as a caller gets it: under the 256 MiB cap of the curve workspace one
                            order takes 181 MB at these shapes, so the call launches the curve kernels ONE order at a time;
  shapley_one_launch        the same call with the cap lifted (_ws_bytes) so that all 8 orders go in one launch of the curve
                            kernels (1.44 GB of workspace): what the cap costs or saves, not what the default call does;
  composition               the only route to the same numbers without this call: 8 explain_faithfulness calls, each with the
                            map -rank of one order (so that the ranking kernel reproduces the order), then the differences,
                            the scatter to positions and the mean over the orders in torch on the device;
  kernel_orders / _single   vqa_occl_curves_orders with M = 8 against 8 launches of vqa_occl_curves (one order each, repeated
                            for every question) on the same U, of every asked image in one buffer;
  kernel_accumulate         vqa_shapley_accumulate alone on the curves of 8 orders.  Byte model: both curves are read once, the
                            table of ranks once per question row (from cache), the state and both results written:
                            (2 * B * M * (P + 1) + 4 * B * P) * 4 bytes.

The driver never touches the GPU: the measurement is a child process under its own `timeout`, and a failure ends the run.
Output: one JSON object on stdout and in OUT_DIR/explain_shapley_bench.json.
"""
import json
import statistics

from bench_explain_common import A, S, SHAPES, T, V, main, setup, window as _window

PERMUTATIONS = 16


def step_time(reps, iters):
    import torch
    from dl_vqa_amd import compact_image_index, ops, shapley_orders
    med = statistics.median
    M = PERMUTATIONS // 2
    res = {"shape": dict(S=S, T=T, A=A, V=V, dtype="fp32", permutations=PERMUTATIONS),
           "method": f"HIP events, interleaved, median of {reps} windows of {iters} calls (kernels: {10 * iters}), 2 warm-up calls "
                     f"per path; composition: {M} explain_faithfulness calls with maps = -rank, then difference, scatter and mean "
                     f"in torch on the device; no hardware counters were collected",
           "cases": []}
    for N, per in SHAPES:
        cs = setup(N, per)
        m, B, q, ql, image_index, feats = cs.m, cs.B, cs.q, cs.ql, cs.image_index, cs.feats
        del cs
        Pn = feats.vn.shape[1]
        dev = feats.vn.device
        table = shapley_orders(PERMUTATIONS, Pn, 0)
        rank = torch.empty_like(table).scatter_(1, table, torch.arange(Pn).expand_as(table))
        fake = [(-rank[i].float()).expand(B, Pn).contiguous().to(dev) for i in range(M)]     # ranks descending: order i
        table_dev = table.to(dev)

        def answer():
            return m.answer(feats, q, ql, image_index)

        def occlusion():
            return m.explain_occlusion(feats, q, ql, image_index)

        def shapley():
            return m.explain_shapley(feats, q, ql, image_index, permutations=PERMUTATIONS)

        one_order = ops._lib.load().vqa_occl_curves_orders_workspace_bytes(B, 1, Pn, m._engine.G, m._engine.hid)

        def shapley_one_launch():
            return m.explain_shapley(feats, q, ql, image_index, permutations=PERMUTATIONS, _ws_bytes=M * one_order)

        def composition():
            total = torch.zeros(B, Pn, device=dev)
            for i in range(M):
                f = m.explain_faithfulness(feats, q, ql, image_index, fake[i])
                steps = 0.5 * ((f.insertion[:, 1:] - f.insertion[:, :-1]) + (f.deletion[:, :-1] - f.deletion[:, 1:]))
                total += torch.zeros_like(steps).scatter_(1, table_dev[i].expand(B, Pn), steps)
            return total / M

        # the kernels alone, on operands of the call's shapes: U of every asked image in one buffer
        eng, P = m._engine, m._param_dict()
        G, hid = eng.G, eng.hid
        rows, slot, _, _ = compact_image_index(image_index, N)
        slot = slot.to(dev)
        R = rows.numel()
        score = 2 * torch.randn(B, G, Pn, device=dev)
        probs = torch.softmax(score, -1)
        U = torch.randn(R, Pn, G, hid, device=dev)
        base = torch.randn(B, hid, device=dev)
        cnull = score.mean(-1).contiguous()
        cols = torch.randint(0, A, (B,), dtype=torch.int32, device=dev)
        orders32, rank32 = table.to(torch.int32).to(dev), rank.to(torch.int32).to(dev)
        single = [orders32[i].expand(B, Pn).contiguous() for i in range(M)]
        out1 = (torch.empty(B, Pn + 1, device=dev), torch.empty(B, Pn + 1, device=dev))
        outM = (torch.empty(B, M, Pn + 1, device=dev), torch.empty(B, M, Pn + 1, device=dev))
        ws1 = ops.occl_curves_workspace(B, Pn, G, hid, dev)
        wsM = ops.occl_curves_orders_workspace(B, M, Pn, G, hid, dev)
        state = (torch.empty(B, Pn, device=dev), torch.empty(B, Pn, device=dev))
        result = (torch.empty(B, Pn, device=dev), torch.empty(B, Pn, device=dev))
        w2, b2 = P["classifier.lin2.weight"], P["classifier.lin2.bias"]

        def kernel_single():
            for i in range(M):
                ops.occl_curves(base, U, slot, probs, score, cnull, w2, b2, cols, single[i], out=out1, workspace=ws1)

        def kernel_orders():
            return ops.occl_curves_orders(base, U, slot, probs, score, cnull, w2, b2, cols, orders32, out=outM, workspace=wsM)

        def kernel_accumulate():
            return ops.shapley_accumulate(*outM, rank32, slot, cols, state, A, R, total=M, out=result)

        paths = {"answer": (answer, iters), "occlusion_w1": (occlusion, iters), "shapley": (shapley, iters),
                 "shapley_one_launch": (shapley_one_launch, iters),
                 "composition": (composition, 1), "kernel_single": (kernel_single, 10 * iters),
                 "kernel_orders": (kernel_orders, 10 * iters), "kernel_accumulate": (kernel_accumulate, 10 * iters)}
        for _ in range(2):
            for fn, _n in paths.values():
                fn()
        torch.cuda.synchronize()
        got, comp = shapley(), composition()
        same_bits = bool(torch.equal(got.maps, shapley_one_launch().maps))
        diff = float((got.maps.reshape(B, Pn) - comp).abs().max())
        gap = float(got.completeness_gap().abs().max())
        t = {k: [] for k in paths}
        for _ in range(reps):
            for k, (fn, n) in paths.items():
                t[k].append(_window(fn, n))
        ms = {k: med(x) for k, x in t.items()}
        acc_bytes = (2 * B * M * (Pn + 1) + 4 * B * Pn) * 4
        case = dict(N=N, questions_per_image=per, B=B, P=Pn, G=G, hid=hid, orders=M,
                    orders_per_launch=min(M, max(1, eng.SHAPLEY_WS_BYTES // (ws1.numel() * 4))),
                    **{k + "_ms": round(x, 3) for k, x in ms.items() if not k.startswith("kernel")},
                    one_launch_over_default=round(ms["shapley_one_launch"] / ms["shapley"], 3), one_launch_maps_bit_equal=same_bits,
                    composition_over_shapley=round(ms["composition"] / ms["shapley"], 2),
                    composition_minus_shapley_ms=round(ms["composition"] - ms["shapley"], 3),
                    shapley_over_answer=round(ms["shapley"] / ms["answer"], 2),
                    shapley_over_occlusion_w1=round(ms["shapley"] / ms["occlusion_w1"], 2),
                    kernel_orders_us=round(1e3 * ms["kernel_orders"], 1), kernel_single_us=round(1e3 * ms["kernel_single"], 1),
                    kernel_orders_over_single=round(ms["kernel_orders"] / ms["kernel_single"], 3),
                    kernel_accumulate_us=round(1e3 * ms["kernel_accumulate"], 1), accumulate_bytes=acc_bytes,
                    kernel_accumulate_TBps=round(acc_bytes / ms["kernel_accumulate"] / 1e9, 3),
                    workspace_bytes_per_order=ws1.numel() * 4,
                    min_max_ms={k: [round(min(x), 3), round(max(x), 3)] for k, x in t.items()},
                    max_abs_shapley_minus_composition=diff, max_abs_completeness_gap=gap,
                    max_abs_map=float(got.maps.abs().max()))
        res["cases"].append(case)
        del m, feats, U, ws1, wsM, outM
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main(__file__, step_time, "explain_shapley_bench.json", iters=3, limit=540)
