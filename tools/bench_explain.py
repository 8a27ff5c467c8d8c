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
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

S, T, A, V = 224, 14, 1000, 5000
SHAPES = [(256, 1), (32, 8)]          # (images, questions per image)


def _window(fn, iters):
    import torch
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters


def step_time(reps, iters):
    import torch
    from dl_vqa_amd import VqaNet, group_by_image, ops
    from oracle import vqa_oracle as O
    from tests.golden_util import full_cfg
    med = statistics.median
    res = {"shape": dict(S=S, T=T, A=A, V=V, dtype="fp32"),
           "method": f"HIP events, interleaved, median of {reps} windows of {iters} calls (kernels: {10 * iters}), 2 warm-up calls "
                     "per path; the forward+backward route's v[image_index] gather is outside its window", "cases": []}
    for N, per in SHAPES:
        torch.manual_seed(1)
        m = VqaNet(full_cfg(A), V).cuda().eval()
        for p in m.parameters():                         # a saliency user freezes the weights: only d logit / d v is computed
            p.requires_grad_(False)
        B = N * per
        v, q, _, _, _, _, ql = O.synthetic_batch(B, S, T, V, A, seed=2)
        v, q, ql = v[:N].cuda(), q.cuda(), ql.cuda()
        image_index = torch.arange(B) % N
        v_rep = v[image_index.cuda()].contiguous().requires_grad_(True)
        feats = m.encode_images(v)
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
        del m, v, v_rep, feats, f16
        torch.cuda.empty_cache()
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--step", choices=["time"], help="internal: run the GPU step in this process")
    a = ap.parse_args()
    if a.step == "time":
        return step_time(a.reps, a.iters)
    os.makedirs(a.out_dir, exist_ok=True)
    cmd = ["timeout", "-k", "10", "420", sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--iters", str(a.iters),
           "--step", "time"]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-4000:] + r.stderr[-4000:])
        raise SystemExit(f"the measurement ended with status {r.returncode}")
    line = json.dumps(json.loads(r.stdout.strip().splitlines()[-1]))
    with open(os.path.join(a.out_dir, "explain_bench.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
