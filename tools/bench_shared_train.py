"""Training through shared image features: the whole train step (forward, fused loss, backward, FusedAdam.step) through
VqaNet.forward_shared / train.run_batch_shared against the same step through model(v[image_index], q, q_len) / run_batch,
the only way to train on such a batch without them.

    python tools/bench_shared_train.py [--out-dir profiles] [--reps 7] [--iters 3] [--no-trace]

North-star architecture, fp32, 224 x 224, T = 14, A = 1000, train mode (every dropout site active); N = 32 images x 8
questions (B = 256) and N = 256 x 1 (nothing to share: the worst case for the new path).  Both paths are timed in ONE
process on one model and one optimiser, interleaved (parent, new, parent, new, ...), with HIP events on the stream after a
warm-up; the figure is the median over --reps windows of --iters steps each.  A second step runs both paths at 32 x 8 under
`rocprofv3 --kernel-trace --stats` (a run of its own, no counters) and writes the kernel table.

The driver itself never touches the GPU: every step is a child process under its own `timeout`, and the first step that
fails ends the run.  Output: one JSON object on stdout and in OUT_DIR/shared_train_bench.json, the kernel table in
OUT_DIR/shared_train_kernel_stats.txt.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_multi_question import _window, run_step  # noqa: E402  (the timing window and the child-process runner)

S, T, A, V = 224, 14, 1000, 5000
SHAPES = [(32, 8), (256, 1)]          # (images, questions per image)


def _setup(N, per):
    import torch
    from dl_vqa_amd import VqaNet
    from dl_vqa_amd.train import FusedAdam, run_batch, run_batch_shared
    from oracle import vqa_oracle as O
    from tests.golden_util import full_cfg
    torch.manual_seed(1)
    m = VqaNet(full_cfg(A), V).cuda().train()
    opt = FusedAdam(m, lr=1e-4)
    B = N * per
    v, q, a_idx, a_val, a_len, idx, ql = O.synthetic_batch(B, S, T, V, A, seed=2)
    v = v[:N].cuda()
    q, ql, a_idx, a_val = q.cuda(), ql.cuda(), a_idx.cuda(), a_val.cuda()
    # question b asks about image b % N: every image has `per` questions, neighbours in the batch differ
    image_index = torch.arange(B) % N
    v_rep = v[image_index.cuda()].contiguous()           # the parent path's input, gathered outside the timed window
    shared = (v, q, a_idx, a_val, a_len, idx, ql)
    gathered = (v_rep, q, a_idx, a_val, a_len, idx, ql)

    def step(loss):
        opt.zero_grad()
        loss.backward()
        opt.step()
        return loss.detach()

    def parent():
        return step(run_batch(m, None, gathered, A)[0])

    def new():
        return step(run_batch_shared(m, shared, A, image_index)[0])

    return m, parent, new


def step_time(reps, iters):
    import torch
    res = {"shape": dict(S=S, T=T, A=A, V=V, dtype="fp32", mode="train"),
           "method": f"whole train step (forward, fused loss, backward, FusedAdam.step); HIP events, interleaved, median of "
                     f"{reps} windows of {iters} steps, 2 warm-up steps per path; the parent's v[image_index] gather is outside "
                     "its window", "cases": []}
    try:
        smi = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=30).stdout
        res["clocks"] = [ln.strip() for ln in smi.splitlines() if "sclk" in ln or "mclk" in ln][:4]
    except Exception as e:                               # noqa: BLE001  (the clocks are a note, not a measurement)
        res["clocks"] = f"not available ({type(e).__name__})"
    for N, per in SHAPES:
        m, parent, new = _setup(N, per)
        B = N * per
        for _ in range(2):
            l_p, l_n = parent(), new()
        torch.cuda.synchronize()
        assert m._last_backward_direct is True
        tp, tn = [], []
        for _ in range(reps):
            tp.append(_window(parent, iters))
            tn.append(_window(new, iters))
        med = statistics.median
        res["cases"].append(dict(
            N=N, questions_per_image=per, B=B, parent_ms=round(med(tp), 3), new_ms=round(med(tn), 3),
            parent_ms_min_max=[round(min(tp), 3), round(max(tp), 3)], new_ms_min_max=[round(min(tn), 3), round(max(tn), 3)],
            parent_samples_per_s=round(B / med(tp) * 1e3, 1), new_samples_per_s=round(B / med(tn) * 1e3, 1),
            speedup=round(med(tp) / med(tn), 3), warmup_loss_parent=float(l_p), warmup_loss_new=float(l_n)))
        del m, parent, new
        torch.cuda.empty_cache()
    print(json.dumps(res))


def step_kernels(iters):
    """What the kernel trace sees: both paths at 32 x 8, `iters` steps each after one warm-up step."""
    import torch
    _, parent, new = _setup(*SHAPES[0])
    for _ in range(iters + 1):
        parent()
        new()
    torch.cuda.synchronize()
    print(json.dumps({"steps_per_path": iters + 1}))


def kernel_table(trace_dir, calls):
    import csv
    import glob
    import re
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
    NT = (P + 15) // 16
    lines = [f"# rocprofv3 --kernel-trace --stats: {calls} train steps through model(v[image_index], q, q_len) and {calls} "
             f"through forward_shared, N = {N} images x {per} questions (B = {B}), 224 x 224, fp32, train mode",
             f"# total kernel time {tot / 1e6:.2f} ms", f"{'kernel':88s}{'calls':>6s}{'avg_us':>11s}{'total_ms':>10s}{'pct':>7s}"]
    picked = {}
    for n, c, t in sorted(rows, key=lambda r: -r[2])[:48]:
        lines.append(f"{short(n):88s}{c:6d}{t / 1e3 / c:11.1f}{t / 1e6:10.3f}{100 * t / tot:7.2f}")
    for n, c, t in rows:
        if "att_score_grouped_bwd" in n:
            picked["grouped_bwd_us"] = t / 1e3 / c
        elif "att_score_bwd_kernel" in n:
            picked["parent_att_score_bwd_us"] = t / 1e3 / c
        elif "att_apply_gather_bwd" in n:
            picked["apply_gather_bwd_us"] = t / 1e3 / c
        elif "att_score_grouped_kernel" in n:
            picked["grouped_drop_fwd_us"] = t / 1e3 / c
    if "grouped_bwd_us" in picked:
        # v' read + dv' written once per image row, q' and dscore read, the dq' and dwx partials written
        nbytes = 2 * N * P * mid * 4 + B * mid * 4 + B * G * P * 4 + B * NT * mid * 4 + N * NT * G * mid * 4
        picked["grouped_bwd_bytes"] = nbytes
        picked["grouped_bwd_TBps"] = round(nbytes / picked["grouped_bwd_us"] / 1e6, 3)
        picked["grouped_bwd_fraction_of_8TBps_hbm_peak"] = round(picked["grouped_bwd_TBps"] / 8.0, 3)
        lines.append(f"# att_score_grouped_bwd: {nbytes / 1e6:.1f} MB (v' in, dv' out, q', dscore, dq' and dwx partials) in "
                     f"{picked['grouped_bwd_us']:.1f} us = {picked['grouped_bwd_TBps']} TB/s; the parent's att_score_bwd at "
                     f"B = {B}: {picked.get('parent_att_score_bwd_us', float('nan')):.1f} us for "
                     f"{2 * B * P * mid * 4 / 1e6:.0f} MB of x read and rewritten")
    return "\n".join(lines) + "\n", {k: (round(v, 2) if isinstance(v, float) else v) for k, v in picked.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=3)
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
        with open(os.path.join(a.out_dir, "shared_train_kernel_stats.txt"), "w") as f:
            f.write(table)
        res["kernel_trace"] = picked
    line = json.dumps(res)
    with open(os.path.join(a.out_dir, "shared_train_bench.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
