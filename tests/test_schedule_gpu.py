"""The engine's per-call schedule switches: VQA_STREAMS, VQA_STREAMS_BWD, VQA_GRAPH, VQA_FUSED_LSTM.

The first three only decide WHERE and HOW the same kernels are launched (one stream or a side stream for the question
branch, where the two are joined, plain launches or a graph replay of the recurrence), so they must not change a bit:
logits, loss, every parameter gradient and the image gradient of a train-mode step (dropout on, the same torch.manual_seed
before each run, so the masks are shared) are compared with torch.equal against VQA_STREAMS=0.  The results are read through
clones enqueued on the current stream right after loss.backward(), BEFORE any synchronize: what a training loop's next
kernel would see.  A missing final join of the side stream is visible that way and not after a device-wide synchronize.
Three steps per schedule, with NaN-filled tensors allocated and freed in between on the main and the side stream, so the
caching allocator hands reused blocks to the next step.

Two shapes make each join the one that is actually waited on: a question branch much longer than the image branch
(north-star widths, H=1024, T=30 on 64x64 images) and the opposite (224x224 images, T=1).

VQA_FUSED_LSTM picks other kernels (a GEMM + cell kernel per step), so its two settings are both held to the CPU oracle.
"""
import functools

import pytest
import torch

from tests.golden_util import full_cfg, tiny_cfg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

SWITCHES = ("VQA_STREAMS", "VQA_STREAMS_BWD", "VQA_GRAPH", "VQA_FUSED_LSTM")
BASELINE = {"VQA_STREAMS": "0"}
SCHEDULES = [
    {"VQA_STREAMS": "1"},
    {"VQA_STREAMS": "2"},
    {"VQA_STREAMS": "2", "VQA_STREAMS_BWD": "1"},
    {"VQA_STREAMS": "1", "VQA_STREAMS_BWD": "2"},
    {"VQA_STREAMS": "2", "VQA_GRAPH": "0"},
]
# name: (B, S, T, q_len)
SHAPES = {
    "long_questions": (5, 64, 30, [30, 1, 17, 30, 8]),
    "large_images": (2, 224, 1, [1, 1]),
}
V, A, STEPS = 2000, 1000, 3


def _sid(env):
    return "-".join(f"{k[4:].lower()}{v}" for k, v in env.items())


class _schedule:
    """the switches set to `env` (the others unset) for the duration of a with block"""

    def __init__(self, env):
        self.env, self.mp = env, pytest.MonkeyPatch()

    def __enter__(self):
        for k in SWITCHES:
            self.mp.delenv(k, raising=False)
        for k, v in self.env.items():
            self.mp.setenv(k, v)

    def __exit__(self, *exc):
        self.mp.undo()


@functools.lru_cache(maxsize=None)
def model():
    from dl_vqa_amd import VqaNet
    torch.manual_seed(17)
    return VqaNet(full_cfg(A), V).to(DEV).train()


@functools.lru_cache(maxsize=None)
def batch(shape):
    from oracle import vqa_oracle as O
    B, S, T, ql = SHAPES[shape]
    v, q, a_idx, a_val, _, _, _ = O.synthetic_batch(B, S, T, V, A, seed=6)
    ql = torch.tensor(ql)
    q = q * (torch.arange(T)[None, :] < ql[:, None])
    return tuple(t.to(DEV) for t in (v, q, ql, a_idx, a_val))


def _churn(m):
    """allocate, poison and free blocks of the sizes a step uses, on the main stream and on the engine's side stream"""
    def junk():
        for n in (1 << 12, 1 << 16, 1 << 20, 5 << 20):
            torch.full((n,), float("nan"), device=DEV)
    junk()
    for side in m._engine._sides.values():
        with torch.cuda.stream(side):
            junk()


def _steps(shape, env, shared=False):
    """STEPS train-mode steps under the schedule `env`; per step the list [logits, loss, image gradient, parameter
    gradients ...] as clones enqueued right behind backward.  No synchronize before the last clone of the last step."""
    from dl_vqa_amd.train import soft_ce_loss_and_score
    m = model()
    v, q, ql, a_idx, a_val = batch(shape)
    index = [b % 2 for b in range(q.shape[0])]                # forward_shared: the questions look at two images
    snaps = []
    with _schedule(env):
        torch.manual_seed(123)                                # the same dropout seeds, step by step, under every schedule
        for _ in range(STEPS):
            vg = (v[:2] if shared else v).clone().requires_grad_()
            y = m.forward_shared(vg, q, ql, index) if shared else m(vg, q, ql)
            loss, _ = soft_ce_loss_and_score(y, a_idx, a_val)
            loss.backward()
            snaps.append([y.detach().clone(), loss.detach().clone(), vg.grad.clone()] + [p.grad.clone() for p in m.parameters()])
            m.zero_grad(set_to_none=True)
            del y, loss, vg
            _churn(m)
    torch.cuda.synchronize()
    return snaps


@functools.lru_cache(maxsize=None)
def baseline(shape, shared=False):
    snaps = _steps(shape, BASELINE, shared)
    for s in snaps:
        assert all(bool(torch.isfinite(t).all()) for t in s)
    assert not torch.equal(snaps[0][0], snaps[1][0])          # dropout draws a new mask per step
    return snaps


def _same(snaps, ref, what):
    names = ["logits", "loss", "image gradient"] + [n for n, _ in model().named_parameters()]
    for step, (a, b) in enumerate(zip(snaps, ref)):
        for name, x, y in zip(names, a, b):
            assert torch.equal(x, y), (f"{what}: {name} of step {step} differs from VQA_STREAMS=0 "
                                       f"(max |diff| {float((x - y).abs().max()):.3e})")


@pytest.mark.parametrize("env", SCHEDULES, ids=_sid)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_schedule_switch_changes_no_bit(shape, env):
    _same(_steps(shape, env), baseline(shape), f"{shape} {_sid(env)}")


@pytest.mark.parametrize("env", [{"VQA_STREAMS": "2"}, {"VQA_STREAMS": "1", "VQA_STREAMS_BWD": "2"}], ids=_sid)
def test_forward_shared_schedule_changes_no_bit(env):
    """forward_shared and its grouped backward have their own fork and join"""
    _same(_steps("long_questions", env, shared=True), baseline("long_questions", True), f"forward_shared {_sid(env)}")


def test_inference_schedule_changes_no_bit():
    """a forward that saves no context (no_grad, eval): the logits, cloned right behind the call"""
    m = model()
    v, q, ql, _, _ = batch("long_questions")
    out = {}
    m.eval()
    try:
        for env in [BASELINE] + SCHEDULES[:2] + SCHEDULES[4:]:
            with _schedule(env), torch.no_grad():
                ys = []
                for _ in range(STEPS):
                    ys.append(m(v, q, ql).clone())
                    _churn(m)
            torch.cuda.synchronize()
            out[_sid(env)] = ys
    finally:
        m.train()
    ref = out[_sid(BASELINE)]
    assert bool(torch.isfinite(ref[0]).all()) and torch.equal(ref[0], ref[1]) and torch.equal(ref[0], ref[2])
    for name, ys in out.items():
        for step, y in enumerate(ys):
            assert torch.equal(y, ref[0]), f"inference under {name}: logits of call {step} differ from VQA_STREAMS=0"


@pytest.mark.parametrize("fused", ["0", "1"])
def test_fused_and_unfused_recurrence_match_the_oracle(fused):
    """H=32 takes either path: VQA_FUSED_LSTM=1 the sequence kernels (one call per pass, a graph each), =0 a recurrent GEMM
    + cell kernel per step.  T=14, ragged lengths incl. 1 and T, bidirectional; both are held to the float64 oracle at the
    bounds of tests/test_model_gpu.py::test_matches_cpu_oracle_on_random_batch."""
    from oracle import vqa_oracle as O
    from dl_vqa_amd import VqaNet, ops
    from dl_vqa_amd.train import soft_ce_loss_and_score
    from tests.test_model_gpu import grad_err
    cfg = tiny_cfg(dict(bidirectional=True, stride=1, do_option="+"))
    cfg["text"]["question_features"] = 32
    T = 14
    torch.manual_seed(11)
    m = VqaNet(cfg, 40).to(DEV).eval()
    v, q, a_idx, a_val, _, _, _ = O.synthetic_batch(5, 48, T, 40, 12, seed=3)
    ql = torch.tensor([14, 1, 9, 5, 14])
    q = q * (torch.arange(T)[None, :] < ql[:, None])
    sd64 = {k: t.double().cpu() for k, t in m.state_dict().items()}
    y_ref, loss_ref, grads_ref = O.loss_and_grads(sd64, cfg, v.double(), q, ql, a_idx, a_val)
    torch.cuda.synchronize()
    before = ops.lstm_graph_stats()
    with _schedule({"VQA_FUSED_LSTM": fused}):
        y = m(v.to(DEV), q.to(DEV), ql.to(DEV))
        loss, _ = soft_ce_loss_and_score(y, a_idx.to(DEV), a_val.to(DEV))
        loss.backward()
    torch.cuda.synchronize()
    after = ops.lstm_graph_stats()
    print(f"[schedule] VQA_FUSED_LSTM={fused}: graph stats (replays, builds, plain, cached) {before} -> {after}")
    if fused == "1":      # one sequence call forward, one backward, each through the graph cache
        assert (after[0] - before[0]) + (after[1] - before[1]) == 2 and after[2] == before[2], (before, after)
    else:                 # no sequence call at all
        assert after == before, (before, after)
    e_y = float((y.detach().cpu().double() - y_ref).abs().max())
    e_l = abs(float(loss) - float(loss_ref))
    worst = max((grad_err(k, p.grad, grads_ref[k]), k) for k, p in m.named_parameters())
    print(f"[parity] VQA_FUSED_LSTM={fused}: logits max abs err {e_y:.3e}, loss err {e_l:.3e}, worst gradient {worst[0]:.3e} ({worst[1]})")
    assert e_y < 1e-5 and e_l < 1e-5
    for k, p in m.named_parameters():
        assert grad_err(k, p.grad, grads_ref[k]) < 1e-4, k
