"""Training on cached image features: the whole train step (forward, fused loss, backward, FusedAdam.step) through
VqaNet.forward_features / train.run_batch_features against the step that runs the image encoder.

    python tools/bench_feature_train.py [--out-dir profiles] [--reps 7] [--iters 3] [--no-trace]

North-star architecture, fp32, 224 x 224, T = 14, A = 1000, train mode (every dropout site active).  Cases:
  (a) 256 questions on 256 distinct rows of a 256-row bank, against run_batch on the same batch (the reference's shuffled
      loader: nothing to share);
  (b) the same batch from a 2 048-row bank (the 256 encoded images repeated 8 times; question b asks about a copy of image b,
      the asked rows spread over the whole bank) -- no kernel depends on the size of the bank, so (b) should equal (a);
  (c) 32 rows x 8 questions, against run_batch_shared.
All paths of a case are timed in ONE process on one model and one optimiser, interleaved, with HIP events on the stream
after 2 warm-up steps per path; the figure is the median over --reps windows of --iters steps each.  The same step times
vqa_gather_rows_drop at 256 x 173 056 against the two passes it replaces (vqa_gather_rows, then vqa_dropout in place),
alternately.  A second step runs the features path of case (a) under `rocprofv3 --kernel-trace --stats` (a run of its own,
no counters) and writes the kernel table; kernels launched fewer times than there are steps (the bank's encoding) are
listed but left out of the per-step figures.

The driver itself never touches the GPU: every step is a child process under its own `timeout`, and the first step that
fails ends the run.  Output: one JSON object on stdout and in OUT_DIR/feature_train_bench.json, the kernel table in
OUT_DIR/feature_train_kernel_stats.txt.
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
B = 256
BANK_COPIES = 8                       # case (b): a bank of 8 x 256 = 2 048 rows
HBM_PEAK_GBPS = 8000.0


def _setup(N):
    """One model, one optimiser, N images and 256 questions (question b asks about image b % N)."""
    import torch
    from dl_vqa_amd import ImageFeatures, VqaNet
    from dl_vqa_amd.train import FusedAdam, run_batch, run_batch_features, run_batch_shared
    from oracle import vqa_oracle as O
    from tests.golden_util import full_cfg
    torch.manual_seed(1)
    m = VqaNet(full_cfg(A), V).cuda().train()
    opt = FusedAdam(m, lr=1e-4)
    v, q, a_idx, a_val, a_len, idx, ql = O.synthetic_batch(B, S, T, V, A, seed=2)
    v = v[:N].cuda()
    q, ql, a_idx, a_val = q.cuda(), ql.cuda(), a_idx.cuda(), a_val.cuda()
    image_index = torch.arange(B) % N
    m.eval()
    feats = m.encode_images(v, with_vprime=False)        # the bank: encoded once, outside every timed window
    m.train()
    bank = ImageFeatures.cat([feats] * BANK_COPIES)      # row r of the bank is image r % N
    bank_index = image_index + N * (torch.arange(B) % BANK_COPIES)
    full = (v[image_index.cuda()].contiguous() if N != B else v, q, a_idx, a_val, a_len, idx, ql)
    shared = (v, q, a_idx, a_val, a_len, idx, ql)
    nov = (None, q, a_idx, a_val, a_len, idx, ql)

    def step(loss):
        opt.zero_grad()
        loss.backward()
        opt.step()
        return loss.detach()

    paths = dict(
        run_batch=lambda: step(run_batch(m, None, full, A)[0]),
        run_batch_shared=lambda: step(run_batch_shared(m, shared, A, image_index)[0]),
        features=lambda: step(run_batch_features(m, nov, A, feats, image_index)[0]),
        features_big_bank=lambda: step(run_batch_features(m, nov, A, bank, bank_index)[0]))
    return m, paths, feats


def _timed(paths, names, reps, iters):
    """Interleaved windows of the named paths: {name: [ms per step of every window]} and the warm-up losses."""
    import torch
    for _ in range(2):
        losses = {n: float(paths[n]()) for n in names}
    torch.cuda.synchronize()
    t = {n: [] for n in names}
    for _ in range(reps):
        for n in names:
            t[n].append(_window(paths[n], iters))
    return t, losses


def _entry(ms):
    med = statistics.median(ms)
    return dict(ms=round(med, 3), ms_min_max=[round(min(ms), 3), round(max(ms), 3)], samples_per_s=round(B / med * 1e3, 1))


def _gather_bench(feats, reps, iters):
    """vqa_gather_rows_drop at 256 rows x 173 056 floats against vqa_gather_rows + vqa_dropout (in place), alternately."""
    import torch
    from dl_vqa_amd import ops
    M, Pn, C = feats.vn.shape
    row_len = Pn * C
    rows = torch.randperm(M, generator=torch.Generator().manual_seed(3)).to(torch.int32).cuda()
    src2d = feats.vn.view(M, row_len)
    dst = torch.empty(M, row_len, device="cuda")
    one = lambda: ops.gather_rows_drop(feats.vn, rows, 0.3, 12345, out=dst)

    def two():
        ops.gather_rows(src2d, rows, dst, row_len)
        ops.dropout(dst, 0.3, 12345, out=dst)

    for _ in range(3):
        one(), two()
    torch.cuda.synchronize()
    t1, t2 = [], []
    for _ in range(reps):
        t1.append(_window(one, 4 * iters))
        t2.append(_window(two, 4 * iters))
    med = statistics.median
    nbytes = 2 * M * row_len * 4
    gbps = nbytes / med(t1) / 1e6
    return dict(n=M, row_len=row_len, p=0.3, bytes=nbytes, one_pass_ms=round(med(t1), 4), two_pass_ms=round(med(t2), 4),
                one_pass_ms_min_max=[round(min(t1), 4), round(max(t1), 4)],
                two_pass_ms_min_max=[round(min(t2), 4), round(max(t2), 4)],
                one_pass_GBps=round(gbps, 1), fraction_of_8TBps_hbm_peak=round(gbps / HBM_PEAK_GBPS, 3),
                speedup_over_two_pass=round(med(t2) / med(t1), 3))


def step_time(reps, iters):
    import torch
    res = {"shape": dict(S=S, T=T, A=A, V=V, B=B, dtype="fp32", mode="train"),
           "method": f"whole train step (forward, fused loss, backward, FusedAdam.step); HIP events, paths interleaved, median "
                     f"of {reps} windows of {iters} steps, 2 warm-up steps per path; the bank is encoded outside every window",
           "cases": {}}
    try:
        smi = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=30).stdout
        res["clocks"] = [ln.strip() for ln in smi.splitlines() if "sclk" in ln or "mclk" in ln][:4]
    except Exception as e:                               # noqa: BLE001  (the clocks are a note, not a measurement)
        res["clocks"] = f"not available ({type(e).__name__})"
    # ---- (a) and (b): 256 distinct images
    m, paths, feats = _setup(B)
    t, losses = _timed(paths, ["run_batch", "features", "features_big_bank"], reps, iters)
    assert m._last_backward_direct is True
    a, b, par = _entry(t["features"]), _entry(t["features_big_bank"]), _entry(t["run_batch"])
    res["cases"]["a_256_rows_of_256"] = dict(rows=B, bank_rows=B, questions=B, run_batch=par, features=a,
                                             speedup_samples_per_s=round(a["samples_per_s"] / par["samples_per_s"], 3),
                                             bar="features >= 2x run_batch samples/s", warmup_losses=losses)
    spread = a["ms_min_max"][1] - a["ms_min_max"][0]
    res["cases"]["b_256_rows_of_2048"] = dict(rows=B, bank_rows=B * BANK_COPIES, questions=B, features=b,
                                              ms_minus_case_a=round(b["ms"] - a["ms"], 3),
                                              case_a_window_spread_ms=round(spread, 3))
    res["gather_rows_drop"] = _gather_bench(feats, reps, iters)
    del m, paths, feats
    torch.cuda.empty_cache()
    # ---- (c): 32 images x 8 questions
    m, paths, feats = _setup(32)
    t, losses = _timed(paths, ["run_batch_shared", "features"], reps, iters)
    c, par = _entry(t["features"]), _entry(t["run_batch_shared"])
    res["cases"]["c_32_rows_x_8"] = dict(rows=32, bank_rows=32, questions=B, run_batch_shared=par, features=c,
                                         speedup_samples_per_s=round(c["samples_per_s"] / par["samples_per_s"], 3),
                                         warmup_losses=losses)
    print(json.dumps(res))


def step_kernels(iters):
    """What the kernel trace sees: the features path of case (a), `iters` steps after one warm-up step (and the encoding of
    the bank, once)."""
    import torch
    _, paths, _ = _setup(B)
    for _ in range(iters + 1):
        paths["features"]()
    torch.cuda.synchronize()
    print(json.dumps({"steps": iters + 1}))


def kernel_table(trace_dir, steps):
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
    # set-up (the bank's encoding: conv blocks, l2norm, a copy; index fills) runs once, so fewer times than there are steps
    setup = sum(t for _, c, t in rows if c < steps)
    lines = [f"# rocprofv3 --kernel-trace --stats: {steps} train steps through run_batch_features (the first is a warm-up step), 256 "
             "questions on 256 distinct rows of a 256-row bank, 224 x 224, fp32, train mode",
             f"# total kernel time {tot / 1e6:.2f} ms, of which {setup / 1e6:.2f} ms in kernels launched fewer than {steps} times: the "
             "bank's encoding, once, before the steps (conv blocks, l2norm_fwd, a copy) -- left out of the per-step figures below",
             f"{'kernel':88s}{'calls':>6s}{'avg_us':>11s}{'total_ms':>10s}{'pct':>7s}"]
    for n, c, t in sorted(rows, key=lambda r: -r[2])[:40]:
        lines.append(f"{short(n):88s}{c:6d}{t / 1e3 / c:11.1f}{t / 1e6:10.3f}{100 * t / tot:7.2f}")
    groups = {"lstm": 0.0, "gemm": 0.0, "att_score_grouped": 0.0, "att_apply": 0.0, "gather_rows_drop": 0.0}
    for n, c, t in rows:
        for k in groups:
            if k in n and c >= steps:
                groups[k] += t
                break
    picked = {k + "_ms_per_step": round(v / 1e6 / steps, 3) for k, v in groups.items()}
    picked["all_kernels_ms_per_step_without_setup"] = round((tot - setup) / 1e6 / steps, 3)
    picked["setup_kernels_ms_once"] = round(setup / 1e6, 3)
    lines.append("# per step, by family (kernel names containing the word; set-up kernels excluded): " + json.dumps(picked))
    return "\n".join(lines) + "\n", picked


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
        with open(os.path.join(a.out_dir, "feature_train_kernel_stats.txt"), "w") as f:
            f.write(table)
        res["kernel_trace"] = picked
    line = json.dumps(res)
    with open(os.path.join(a.out_dir, "feature_train_bench.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
