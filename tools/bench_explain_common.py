"""What the seven explain benchmarks (tools/bench_explain*.py) share: the shapes, the timed window, the set-up of a case and the
driver, which never touches the GPU -- the measurement is a child process under its own `timeout`, a failure ends the run, and
the last line the child prints is the result."""
import argparse
import json
import os
import subprocess
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

S, T, A, V = 224, 14, 1000, 5000
SHAPES = [(256, 1), (32, 8)]          # (images, questions per image)


def window(fn, iters):
    import torch
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters


def setup(N, per, questions_on_device=True):
    """One case: the north-star model in eval mode, B = N * per synthetic questions (on the host where a tool edits them first),
    the N images on the device, image_index = arange(B) % N and the fp32 cache."""
    import torch
    from dl_vqa_amd import VqaNet
    from oracle import vqa_oracle as O
    from tests.golden_util import full_cfg
    torch.manual_seed(1)
    m = VqaNet(full_cfg(A), V).cuda().eval()
    B = N * per
    v, q, _, _, _, _, ql = O.synthetic_batch(B, S, T, V, A, seed=2)
    v = v[:N].cuda()
    if questions_on_device:
        q, ql = q.cuda(), ql.cuda()
    return SimpleNamespace(m=m, B=B, v=v, q=q, ql=ql, image_index=torch.arange(B) % N, feats=m.encode_images(v))


def main(tool, step_time, out_name, iters, limit):
    """The driver of the benchmark in the file `tool`: step_time(reps, iters) in a child under `timeout -k 10 <limit>`, its last
    JSON line on stdout and in OUT_DIR/<out_name>."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=iters)
    ap.add_argument("--step", choices=["time"], help="internal: run the GPU step in this process")
    a = ap.parse_args()
    if a.step == "time":
        return step_time(a.reps, a.iters)
    os.makedirs(a.out_dir, exist_ok=True)
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(tool), "--reps", str(a.reps), "--iters", str(a.iters),
           "--step", "time"]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-4000:] + r.stderr[-4000:])
        raise SystemExit(f"the measurement ended with status {r.returncode}")
    line = json.dumps(json.loads(r.stdout.strip().splitlines()[-1]))
    with open(os.path.join(a.out_dir, out_name), "w") as f:
        f.write(line + "\n")
    print(line)
