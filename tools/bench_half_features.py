"""Float16 image-feature caches against fp32 caches: the kernels that read a cache, the run_batch_features train step and
answer(), each on the same values in both storage formats.

    python tools/bench_half_features.py [--out-dir profiles] [--reps 9] [--iters 5]

North-star architecture, fp32, 224 x 224, T = 14, A = 1000.  Two shapes: 256 questions on 256 distinct rows (the shape of
tools/bench_feature_train.py) and 32 rows x 8 questions (tools/bench_multi_question.py).  The images are encoded once into an
fp32 cache (vn and v'); the float16 cache is that cache's .to(torch.float16).  Per shape, with the fp32 and the float16 operand
alternating window by window in ONE process (HIP events on the stream, 3 warm-up calls per path; median and min / max of
--reps windows of --iters calls):
  kernels: vqa_gather_rows_drop (p = 0.3, the asked rows), vqa_att_apply_gather_fwd, vqa_att_apply_gather_dscore,
           vqa_att_score_grouped_fwd -- with the cache bytes each call reads (the byte model: half for float16);
  step:    the whole train step of train.run_batch_features (forward, fused loss, backward, FusedAdam.step), train mode;
  answer:  VqaNet.answer in eval mode.
"slower": whether the float16 median lies above the fp32 median by more than the fp32 windows' own spread (max - min).
Resident cache bytes per image come from the tool's own tensors.

The driver itself never touches the GPU: the measurement is a child process under its own `timeout`.  Output: one JSON object
on stdout and in OUT_DIR/half_features_bench.json.
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
SHAPES = [(256, 1), (32, 8)]          # (rows, questions per row)


def _pair(t32, t16):
    """Medians and spread of the two alternating sample sets."""
    med = statistics.median
    spread = max(t32) - min(t32)
    return dict(fp32_ms=round(med(t32), 4), fp16_ms=round(med(t16), 4),
                fp32_ms_min_max=[round(min(t32), 4), round(max(t32), 4)], fp16_ms_min_max=[round(min(t16), 4), round(max(t16), 4)],
                fp16_over_fp32=round(med(t16) / med(t32), 3), slower=bool(med(t16) > med(t32) + spread))


def _alternate(f32, f16, reps, iters):
    import torch
    for _ in range(3):
        f32(), f16()
    torch.cuda.synchronize()
    t32, t16 = [], []
    for _ in range(reps):
        t32.append(_window(f32, iters))
        t16.append(_window(f16, iters))
    return _pair(t32, t16)


def _shape(N, per, reps, iters):
    import torch
    from dl_vqa_amd import VqaNet, group_by_image, ops
    from dl_vqa_amd.train import FusedAdam, run_batch_features
    from oracle import vqa_oracle as O
    from tests.golden_util import full_cfg
    torch.manual_seed(1)
    m = VqaNet(full_cfg(A), V).cuda().eval()
    opt = FusedAdam(m, lr=1e-4)
    B = N * per
    v, q, a_idx, a_val, a_len, idx, ql = O.synthetic_batch(B, S, T, V, A, seed=2)
    q, ql, a_idx, a_val = q.cuda(), ql.cuda(), a_idx.cuda(), a_val.cuda()
    image_index = torch.arange(B) % N
    parts = [m.encode_images(v[i:i + 32].cuda()) for i in range(0, N, 32)]       # the fp32 temporaries stay at chunk size
    f32 = type(parts[0]).cat(parts)
    f16 = f32.to(torch.float16)
    del parts
    out = dict(rows=N, questions=B)
    out["cache_bytes_per_image"] = {
        "fp32": dict(vn=f32.vn.numel() * f32.vn.element_size() // N, vprime=f32.vprime.numel() * f32.vprime.element_size() // N),
        "fp16": dict(vn=f16.vn.numel() * f16.vn.element_size() // N, vprime=f16.vprime.numel() * f16.vprime.element_size() // N)}

    # ---- the kernels that read a cache, on the operands the schedules give them
    eng = m._engine
    G, C, mid, Pn = eng.G, eng.C, eng.mid, f32.vn.shape[1]
    gen = torch.Generator().manual_seed(3)
    order, offsets = (t.cuda() for t in group_by_image(image_index, N))
    img = image_index.to(torch.int32).cuda()
    rows = torch.arange(N, dtype=torch.int32).cuda()
    score = torch.randn(B, G, Pn, generator=gen).cuda()
    probs = torch.softmax(score, dim=-1)
    Dc = eng.Dc
    comb = torch.empty(B, Dc, device="cuda")
    dcomb = torch.randn(B, Dc, generator=gen).cuda()
    qp = torch.randn(B, mid, generator=gen).cuda()
    wx = m.attention.x_conv.weight.detach().view(G, -1)
    bx = m.attention.x_conv.bias.detach()
    dst = torch.empty(N, Pn, C, device="cuda")
    vn_elems, vp_elems = N * Pn * C, N * Pn * mid                                 # elements read once per call
    kernels = {}

    def kernel(name, fn, elements):
        r = _alternate(lambda: fn(f32), lambda: fn(f16), reps, 4 * iters)
        r["cache_bytes_read"] = dict(fp32=4 * elements, fp16=2 * elements)
        r["cache_GBps"] = dict(fp32=round(4 * elements / r["fp32_ms"] / 1e6, 1), fp16=round(2 * elements / r["fp16_ms"] / 1e6, 1))
        kernels[name] = r

    kernel("gather_rows_drop", lambda f: ops.gather_rows_drop(f.vn, rows, 0.3, 12345, out=dst), vn_elems)
    kernel("att_apply_gather_fwd", lambda f: ops.att_apply_gather_fwd(score, f.vn, img, comb, Dc), vn_elems * per)
    kernel("att_apply_gather_dscore", lambda f: ops.att_apply_gather_dscore(dcomb, Dc, probs, f.vn, img), vn_elems * per)
    kernel("att_score_grouped_fwd", lambda f: ops.att_score_grouped_fwd(f.vprime, qp, wx, bx, order, offsets, N, B, Pn,
                                                                        eng.att_mode), vp_elems)
    out["kernels"] = kernels

    # ---- answer(), eval mode
    out["answer"] = _alternate(lambda: m.answer(f32, q, ql, image_index), lambda: m.answer(f16, q, ql, image_index), reps, iters)

    # ---- the train step on a bank (vn only is read), train mode
    m.train()
    nov = (None, q, a_idx, a_val, a_len, idx, ql)

    def step(feats):
        loss = run_batch_features(m, nov, A, feats, image_index)[0]
        opt.zero_grad()
        loss.backward()
        opt.step()

    out["run_batch_features_step"] = _alternate(lambda: step(f32), lambda: step(f16), reps, iters)
    return out


def step_time(reps, iters):
    import torch
    res = {"shape": dict(S=S, T=T, A=A, V=V, dtype="fp32"),
           "method": f"HIP events, fp32 and float16 operands alternating window by window in one process, median and min / max of "
                     f"{reps} windows of {iters} calls (kernels: {4 * iters}), 3 warm-up calls per path; slower = the float16 median "
                     "above the fp32 median by more than the fp32 windows' max - min",
           "cases": []}
    try:
        smi = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=30).stdout
        res["clocks"] = [ln.strip() for ln in smi.splitlines() if "sclk" in ln or "mclk" in ln][:4]
    except Exception as e:                               # noqa: BLE001  (the clocks are a note, not a measurement)
        res["clocks"] = f"not available ({type(e).__name__})"
    for N, per in SHAPES:
        res["cases"].append(_shape(N, per, reps, iters))
        torch.cuda.empty_cache()
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
    line = json.dumps(json.loads(run_step(me + ["--step", "time"], 540).strip().splitlines()[-1]))
    with open(os.path.join(a.out_dir, "half_features_bench.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
