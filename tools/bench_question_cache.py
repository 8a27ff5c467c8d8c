"""Cached question features: VqaNet.answer_pairs (image cache + question cache) against VqaNet.answer on the expanded
questions, answer(feats, q_u[question_index], q_len_u[question_index], image_index) -- the only way to do the same job
without the question cache.  Both calls read the same warm image features; the image encoder is outside every window.

    python tools/bench_question_cache.py [--out-dir profiles] [--reps 7] [--iters 5]

North-star architecture, fp32, 224 x 224, T = 14, A = 1000.  Cases:
  * 32 images x 8 questions each (B = 256) drawn from 64 distinct questions;
  * 1 question against 1024 images (retrieval);
  * B = 256 pairs, 256 images, 256 distinct questions, nothing repeats -- the case where the new path must not lose.
Per case two figures for the new path: `pairs_ms` with warm question features, and `encode_pairs_ms` with encode_questions
inside the timed window.  Both paths are timed in ONE process, interleaved, with HIP events on the stream after a warm-up;
each figure is the median over --reps windows of --iters calls.

The driver itself never touches the GPU: the measurement is a child process under its own `timeout`.  Output: one JSON
object on stdout and in OUT_DIR/question_cache_bench.json.
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
# (name, images N, pairs B, distinct questions M)
CASES = [("32x8_of_64", 32, 256, 64), ("1_question_x_1024_images", 1024, 1024, 1), ("no_repeats_256", 256, 256, 256)]
ENCODE_CHUNK = 128          # images per encode_images call while the image cache is filled (outside every window)


def _setup(m, N, B, M):
    import torch
    from dl_vqa_amd import ImageFeatures
    from oracle import vqa_oracle as O
    _, q, _, _, _, _, ql = O.synthetic_batch(M, 8, T, V, A, seed=2)
    g = torch.Generator().manual_seed(3)
    parts = [m.encode_images(torch.randn(min(ENCODE_CHUNK, N - n0), 3, S, S, generator=g).cuda())
             for n0 in range(0, N, ENCODE_CHUNK)]
    feats = ImageFeatures(torch.cat([p.vn for p in parts]), torch.cat([p.vprime for p in parts]), parts[0].grid, m)
    image_index = torch.arange(B) % N                    # every image has B / N pairs, neighbours in the batch differ
    question_index = torch.arange(B) % M if M == B or M == 1 else torch.randint(0, M, (B,), generator=g)
    return feats, q, ql, image_index, question_index


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
    from dl_vqa_amd import VqaNet
    from tests.golden_util import full_cfg
    res = {"shape": dict(S=S, T=T, A=A, V=V, dtype="fp32"), "method": f"HIP events, interleaved, median of {reps} windows of "
           f"{iters} calls, 2 warm-up calls per path; image features warm for both paths; answer_ms: answer() on the expanded "
           "questions; pairs_ms: answer_pairs() with warm question features; encode_pairs_ms: encode_questions + answer_pairs",
           "cases": []}
    torch.manual_seed(1)
    m = VqaNet(full_cfg(A), V).cuda().eval()
    for name, N, B, M in CASES:
        feats, q_u, ql_u, image_index, question_index = _setup(m, N, B, M)
        q_u, ql_u = q_u.cuda(), ql_u.cuda()
        q_exp, ql_exp = q_u[question_index.cuda()].contiguous(), ql_u[question_index.cuda()].contiguous()   # outside the windows
        qfeats = [m.encode_questions(q_u, ql_u)]

        def answer():
            return m.answer(feats, q_exp, ql_exp, image_index)

        def pairs():
            return m.answer_pairs(feats, qfeats[0], image_index, question_index)

        def encode_pairs():
            qfeats[0] = m.encode_questions(q_u, ql_u)
            return pairs()

        for _ in range(2):
            y_a, y_p, _ = answer(), pairs(), encode_pairs()
        torch.cuda.synchronize()
        err = float((y_a - y_p).abs().max())
        ta, tp, te = [], [], []
        for _ in range(reps):
            ta.append(_window(answer, iters))
            tp.append(_window(pairs, iters))
            te.append(_window(encode_pairs, iters))
        med = statistics.median
        mm = lambda t: [round(min(t), 3), round(max(t), 3)]
        res["cases"].append(dict(case=name, N=N, B=B, M=M, answer_ms=round(med(ta), 3), pairs_ms=round(med(tp), 3),
                                 encode_pairs_ms=round(med(te), 3), answer_ms_min_max=mm(ta), pairs_ms_min_max=mm(tp),
                                 encode_pairs_ms_min_max=mm(te), speedup_warm=round(med(ta) / med(tp), 3),
                                 speedup_with_encode=round(med(ta) / med(te), 3), logits_max_abs_diff=err))
        del feats, qfeats
        torch.cuda.empty_cache()
    print(json.dumps(res))


def run_step(cmd, seconds):
    """One child process under its own time limit; a failure ends the whole run."""
    r = subprocess.run(["timeout", "-k", "10", str(seconds)] + cmd, capture_output=True, text=True, cwd=ROOT)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-4000:] + r.stderr[-4000:])
        raise SystemExit(f"step {' '.join(cmd[-3:])} ended with status {r.returncode}: nothing further is started")
    return r.stdout


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
    me = [sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--iters", str(a.iters)]
    line = json.dumps(json.loads(run_step(me + ["--step", "time"], 420).strip().splitlines()[-1]))
    with open(os.path.join(a.out_dir, "question_cache_bench.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
