"""Many questions per image: VqaNet.encode_images + answer against the one-image-per-question forward,
model(v[image_index], q, q_len) under torch.no_grad() in eval mode (the only way to do the same job without them).

    python tools/bench_multi_question.py [--out-dir profiles] [--reps 7] [--iters 5] [--no-trace]

North-star architecture, fp32, 224 x 224, T = 14, A = 1000; N = 32 images x 8 questions (B = 256) and N = 256 x 1 (the
worst case for the new path).  Both paths are timed in ONE process, interleaved (parent, new, parent, new, ...), with
HIP events on the stream after a warm-up; the figure is the median over --reps windows of --iters calls each.  A second
step runs both paths under `rocprofv3 --kernel-trace --stats` (a run of its own, no counters) and writes the kernel table.

The driver itself never touches the GPU: every step is a child process under its own `timeout`, and the first step that
fails ends the run.  Output: one JSON object on stdout and in OUT_DIR/multi_question_bench.json, the kernel table in
OUT_DIR/multi_question_kernel_stats.txt.
"""
import argparse
import csv
import glob
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

S, T, A, V = 224, 14, 1000, 5000
SHAPES = [(32, 8), (256, 1)]          # (images, questions per image)


def _setup(N, per):
    import torch
    from dl_vqa_amd import VqaNet
    from oracle import vqa_oracle as O
    from tests.golden_util import full_cfg
    torch.manual_seed(1)
    m = VqaNet(full_cfg(A), V).cuda().eval()
    B = N * per
    v, q, _, _, _, _, ql = O.synthetic_batch(B, S, T, V, A, seed=2)
    v = v[:N].cuda()
    q, ql = q.cuda(), ql.cuda()
    # question b asks about image b % N: every image has `per` questions, neighbours in the batch differ
    image_index = torch.arange(B) % N
    v_rep = v[image_index.cuda()].contiguous()           # the parent path's input, gathered outside the timed window
    return m, v, v_rep, q, ql, image_index


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
    res = {"shape": dict(S=S, T=T, A=A, V=V, dtype="fp32"), "method": f"HIP events, interleaved, median of {reps} windows of "
           f"{iters} calls, 2 warm-up calls per path; the parent's v[image_index] gather is outside its window", "cases": []}
    try:
        smi = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=30).stdout
        res["clocks"] = [ln.strip() for ln in smi.splitlines() if "sclk" in ln or "mclk" in ln][:4]
    except Exception as e:                               # noqa: BLE001  (the clocks are a note, not a measurement)
        res["clocks"] = f"not available ({type(e).__name__})"
    for N, per in SHAPES:
        m, v, v_rep, q, ql, image_index = _setup(N, per)
        B = N * per
        feats = [None]

        def parent():
            with torch.no_grad():
                return m(v_rep, q, ql)

        def encode():
            feats[0] = m.encode_images(v)

        def answer():
            return m.answer(feats[0], q, ql, image_index)

        def new():
            encode()
            return answer()

        for _ in range(2):
            y_p, y_n = parent(), new()
        torch.cuda.synchronize()
        err = float((y_p - y_n).abs().max())
        tp, tn, te, ta = [], [], [], []
        for _ in range(reps):
            tp.append(_window(parent, iters))
            tn.append(_window(new, iters))
            te.append(_window(encode, iters))
            ta.append(_window(answer, iters))
        med = statistics.median
        case = dict(N=N, questions_per_image=per, B=B, parent_ms=round(med(tp), 3), new_ms=round(med(tn), 3),
                    encode_ms=round(med(te), 3), answer_ms=round(med(ta), 3),
                    parent_ms_min_max=[round(min(tp), 3), round(max(tp), 3)], new_ms_min_max=[round(min(tn), 3), round(max(tn), 3)],
                    parent_samples_per_s=round(B / med(tp) * 1e3, 1), new_samples_per_s=round(B / med(tn) * 1e3, 1),
                    speedup=round(med(tp) / med(tn), 3), logits_max_abs_diff=err)
        res["cases"].append(case)
        del m, v, v_rep, feats
        torch.cuda.empty_cache()
    print(json.dumps(res))


def step_kernels(iters):
    """What the kernel trace sees: both paths at 32 x 8, `iters` calls each after one warm-up call."""
    import torch
    m, v, v_rep, q, ql, image_index = _setup(*SHAPES[0])
    for k in range(iters + 1):
        with torch.no_grad():
            m(v_rep, q, ql)
        m.answer(m.encode_images(v), q, ql, image_index)
    torch.cuda.synchronize()
    print(json.dumps({"calls_per_path": iters + 1}))


def kernel_table(trace_dir, calls):
    rows = []
    for f in glob.glob(trace_dir + "/**/*kernel_stats.csv", recursive=True):
        with open(f) as fh:
            for r in csv.DictReader(fh):
                rows.append((r["Name"], int(r["Calls"]), float(r["TotalDurationNs"])))
    if not rows:                                         # rocprofv3's default output is a rocpd SQLite database
        import sqlite3
        for f in glob.glob(trace_dir + "/**/*_results.db", recursive=True):
            c = sqlite3.connect(f)
            tables = [t for (t,) in c.execute("select name from sqlite_master where type in ('table','view')")]
            kt = "kernels" if "kernels" in tables else next((t for t in tables if t.startswith("kernels")), None)
            if kt:
                rows += [(n, int(k), float(t)) for n, k, t in
                         c.execute(f"select name, count(*), sum(duration) from {kt} group by name")]
    if not rows:
        raise SystemExit("no kernel statistics under " + trace_dir)

    def short(n):
        return re.sub(r"\(.*$", "", n.replace("vqa::", "").replace("void ", ""))[:86]

    tot = sum(r[2] for r in rows)
    N, per = SHAPES[0]
    B, P, mid, G = N * per, 26 * 26, 1024, 2
    lines = [f"# rocprofv3 --kernel-trace --stats: {calls} calls of model(v[image_index], q, q_len) and {calls} of "
             f"encode_images + answer, N = {N} images x {per} questions (B = {B}), 224 x 224, fp32, eval mode",
             f"# total kernel time {tot / 1e6:.2f} ms", f"{'kernel':88s}{'calls':>6s}{'avg_us':>11s}{'total_ms':>10s}{'pct':>7s}"]
    picked = {}
    for n, c, t in sorted(rows, key=lambda r: -r[2])[:40]:
        lines.append(f"{short(n):88s}{c:6d}{t / 1e3 / c:11.1f}{t / 1e6:10.3f}{100 * t / tot:7.2f}")
    for n, c, t in rows:
        if "att_score_grouped" in n:
            picked["grouped_us"] = t / 1e3 / c
        elif "att_score_fwd" in n:
            picked["parent_att_score_fwd_us"] = t / 1e3 / c
    if "grouped_us" in picked:
        nbytes = N * P * mid * 4 + B * mid * 4 + B * G * P * 4
        picked["grouped_bytes"] = nbytes
        picked["grouped_TBps"] = round(nbytes / picked["grouped_us"] / 1e6, 3)
        picked["grouped_fraction_of_8TBps_hbm_peak"] = round(picked["grouped_TBps"] / 8.0, 3)
        lines.append(f"# att_score_grouped: {nbytes / 1e6:.1f} MB (v' once per image + q' + scores) in {picked['grouped_us']:.1f} us "
                     f"= {picked['grouped_TBps']} TB/s; the parent's att_score_fwd at B = {B}: "
                     f"{picked.get('parent_att_score_fwd_us', float('nan')):.1f} us for {B * P * mid * 4 / 1e6:.0f} MB of x")
    return "\n".join(lines) + "\n", {k: (round(v, 2) if isinstance(v, float) else v) for k, v in picked.items()}


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
    ap.add_argument("--no-trace", action="store_true", help="skip the rocprofv3 kernel-trace step")
    ap.add_argument("--step", choices=["time", "kernels"], help="internal: run one GPU step in this process")
    a = ap.parse_args()
    if a.step == "time":
        return step_time(a.reps, a.iters)
    if a.step == "kernels":
        return step_kernels(a.iters)
    os.makedirs(a.out_dir, exist_ok=True)
    me = [sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--iters", str(a.iters)]
    res = json.loads(run_step(me + ["--step", "time"], 420).strip().splitlines()[-1])
    if not a.no_trace:
        with tempfile.TemporaryDirectory(dir=a.out_dir) as td:
            run_step(["rocprofv3", "--kernel-trace", "--stats", "-f", "csv", "-d", td, "--"] + me + ["--step", "kernels"], 420)
            table, picked = kernel_table(td, a.iters + 1)
        with open(os.path.join(a.out_dir, "multi_question_kernel_stats.txt"), "w") as f:
            f.write(table)
        res["kernel_trace"] = picked
    line = json.dumps(res)
    with open(os.path.join(a.out_dir, "multi_question_bench.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
