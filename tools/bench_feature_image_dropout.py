"""Image dropout when training on cached image features: the run_batch_features train step with the flag off and on, and the
kernel that applies it (vqa_gather_rows_drop_norm) against its byte model and against vqa_l2norm_fwd on the same rows.

    python tools/bench_feature_image_dropout.py [--out-dir profiles] [--reps 9] [--iters 5]

North-star architecture, fp32, 224 x 224, T = 14, A = 1000, train mode, 256 questions on 256 distinct rows of a 256-row bank
(the shape of tools/bench_feature_train.py), the bank stored as fp32 and as float16.  In ONE process, the paths alternating
window by window (HIP events on the stream, 3 warm-up calls per path; median and min / max of --reps windows of --iters calls):
  step:   the whole train step of train.run_batch_features (forward, fused loss, backward, FusedAdam.step) with
          image_dropout=False and image_dropout=True, per storage format.  The flag-off step runs the code it ran before the
          flag existed: compare its figure with the same tool's "off" figure on the parent commit's tree
          (tools/bench_feature_train.py case (a) measures the same step there).
  kernel: vqa_gather_rows_drop_norm with both outputs (p = p2 = 0.3) on the 256 asked rows, per storage format, alternating
          with vqa_l2norm_fwd with a second output on the same rows x C -- the existing kernel with the same work per element
          (it reads fp32 and also writes one norm per row).  Byte model of the new kernel: reads n*P*C*esz, writes 2*n*P*C*4.
          "below_l2norm": its achieved bandwidth lies below vqa_l2norm_fwd's by more than that kernel's own spread.

The driver itself never touches the GPU: the measurement is a child process under its own `timeout`.  Output: one JSON object
on stdout and in OUT_DIR/feature_image_dropout_bench.json.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_multi_question import _window, run_step  # noqa: E402  (the timing window and the child-process runner)

S, T, A, V = 224, 14, 1000, 5000
N = 256                                # questions = distinct rows


def _stats(ts):
    return dict(ms=round(statistics.median(ts), 4), ms_min_max=[round(min(ts), 4), round(max(ts), 4)])


def _alternate(fns, reps, iters):
    """{name: window times} of the paths `fns`, alternating window by window."""
    import torch
    for _ in range(3):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            ts[k].append(_window(f, iters))
    return ts


def step_time(reps, iters):
    import torch
    from dl_vqa_amd import VqaNet, ops
    from dl_vqa_amd.train import FusedAdam, run_batch_features
    from oracle import vqa_oracle as O
    from tests.golden_util import full_cfg
    res = {"shape": dict(S=S, T=T, A=A, V=V, dtype="fp32", rows=N, questions=N),
           "method": f"HIP events, paths alternating window by window in one process, median and min / max of {reps} windows of "
                     f"{iters} calls (kernels: {4 * iters}), 3 warm-up calls per path"}
    try:
        smi = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=30).stdout
        res["clocks"] = [ln.strip() for ln in smi.splitlines() if "sclk" in ln or "mclk" in ln][:4]
    except Exception as e:                               # noqa: BLE001  (the clocks are a note, not a measurement)
        res["clocks"] = f"not available ({type(e).__name__})"
    torch.manual_seed(1)
    m = VqaNet(full_cfg(A), V).cuda().eval()
    opt = FusedAdam(m, lr=1e-4)
    v, q, a_idx, a_val, a_len, idx, ql = O.synthetic_batch(N, S, T, V, A, seed=2)
    q, ql, a_idx, a_val = q.cuda(), ql.cuda(), a_idx.cuda(), a_val.cuda()
    image_index = torch.arange(N)
    parts = [m.encode_images(v[i:i + 32].cuda(), with_vprime=False) for i in range(0, N, 32)]
    banks = {"fp32": type(parts[0]).cat(parts)}
    banks["fp16"] = banks["fp32"].to(torch.float16)
    del parts
    m.train()
    assert m._engine.p_image == 0.3 and m._engine.p_att == 0.3

    # ---- the train step, flag off and on
    nov = (None, q, a_idx, a_val, a_len, idx, ql)
    takes_flag = "image_dropout" in run_batch_features.__code__.co_varnames      # the parent commit's tree has no such argument

    def step(feats, **kw):
        loss = run_batch_features(m, nov, A, feats, image_index, **kw)[0]
        opt.zero_grad()
        loss.backward()
        opt.step()

    fns = {}
    for fmt, bank in banks.items():
        fns[f"{fmt}_off"] = (lambda b: lambda: step(b))(bank)
        if takes_flag:
            fns[f"{fmt}_on"] = (lambda b: lambda: step(b, image_dropout=True))(bank)
    ts = _alternate(fns, reps, iters)
    res["run_batch_features_step"] = {k: _stats(t) for k, t in ts.items()}
    for fmt in banks:
        if takes_flag:
            off, on = ts[f"{fmt}_off"], ts[f"{fmt}_on"]
            res["run_batch_features_step"][f"{fmt}_on_minus_off_ms"] = round(statistics.median(on) - statistics.median(off), 4)
    if not hasattr(ops, "gather_rows_drop_norm"):
        print(json.dumps(res))
        return

    # ---- the kernel alone, against its byte model and against vqa_l2norm_fwd on the same rows x C
    vn = banks["fp32"].vn
    Pn, C = vn.shape[1], vn.shape[2]
    rows = torch.arange(N, dtype=torch.int32).cuda()
    elems = N * Pn * C
    pooled = vn.view(N * Pn, C)
    kf = {"l2norm_fwd": lambda: ops.l2norm_fwd(pooled, 0.3, 12345, drop2=(0.3, 54321, torch.float32))}
    for fmt, bank in banks.items():
        kf[f"drop_norm_{fmt}"] = (lambda b: lambda: ops.gather_rows_drop_norm(b.vn, rows, 0.3, 12345, drop2=(0.3, 54321)))(bank)
    kt = _alternate(kf, reps, 4 * iters)
    model = {"l2norm_fwd": elems * 4 + 2 * elems * 4 + N * Pn * 4, "drop_norm_fp32": elems * 4 + 2 * elems * 4,
             "drop_norm_fp16": elems * 2 + 2 * elems * 4}
    kernels = {}
    for k, t in kt.items():
        kernels[k] = dict(_stats(t), bytes=model[k], GBps=round(model[k] / statistics.median(t) / 1e6, 1),
                          GBps_min_max=[round(model[k] / max(t) / 1e6, 1), round(model[k] / min(t) / 1e6, 1)])
    ref = kernels["l2norm_fwd"]
    for fmt in banks:
        k = kernels[f"drop_norm_{fmt}"]
        k["GBps_over_l2norm"] = round(k["GBps"] / ref["GBps"], 3)
        k["below_l2norm"] = bool(k["GBps"] < ref["GBps"] - (ref["GBps_min_max"][1] - ref["GBps_min_max"][0]))
    res["kernel"] = dict(rows_x_C=[N * Pn, C], p=0.3, p2=0.3, **kernels)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--step", choices=["time"], help="internal: run the GPU step in this process")
    a = ap.parse_args()
    if a.step == "time":
        return step_time(a.reps, a.iters)
    os.makedirs(a.out_dir, exist_ok=True)
    me = [sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--iters", str(a.iters)]
    line = json.dumps(json.loads(run_step(me + ["--step", "time"], 360).strip().splitlines()[-1]))
    with open(os.path.join(a.out_dir, "feature_image_dropout_bench.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
