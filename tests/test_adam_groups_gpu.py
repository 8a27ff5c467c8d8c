"""GPU: vqa_adam_segments against vqa_adam (same bits on every zero-decay segment, nothing touched between segments),
against torch.optim.Adam / AdamW in float64 where a segment decays, and FusedAdam(groups=...) through the two-phase recipe
(train on a feature bank with the image encoder frozen, then unfreeze it) on the tiny_plus fixture."""
import math
import os
import re

import pytest
import torch

from tests import adam_groups_ref as A
from tests.golden_util import Golden, tiny_cfg
from tests.test_feature_train_gpu import BANK_INDEX, _bank_batch, _encode
from tests.test_model_gpu import build
from tests.test_shared_train_gpu import QSEL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

N = 8192 * 256 + 260                     # floats in each buffer
NAN_BITS = {"p": 0x7FC00A01, "g": 0x7FC00A02, "m": 0x7FC00A03, "v": 0x7FC00A04}      # what lies between the segments


def _ops():
    from dl_vqa_amd import ops
    return ops


def walk_cap():
    """Floats one sweep of the capped grid covers, from the header the kernel is compiled against: blocks x 256 lanes x 4."""
    text = open(os.path.join(ROOT, "include", "vqa_hip.h")).read()
    return int(re.search(r"^#define\s+VQA_ADAM_SEGMENTS_MAX_BLOCKS\s+(\d+)", text, flags=re.M).group(1)) * 256 * 4


def layout(count):
    """Sorted, disjoint [begin, end) ranges.  The walk starts at the first begin (64, not 0), so it wraps at W = 64 + cap.
    7: lengths 4, 64, 68 and 1024; two adjacent pairs (they get different lr and step); one range across W; the last one ends
    at N.  64: the same with 57 more ranges of those four lengths in between.  1: one range from 64 to N (across W)."""
    cap = walk_cap()
    assert N > cap + 64 and N % 4 == 0                     # the grid-stride loop takes a second trip
    W = 64 + cap
    if count == 1:
        return [(64, N)]
    head = [(64, 68), (1000, 1064), (1064, 1132)]
    tail = [(500000, 501024), (W - 40, W + 28), (W + 28, W + 92), (N - 68, N)]
    mid = []
    if count == 64:
        mid = [(2000 + 8000 * i, 2000 + 8000 * i + (4, 64, 68, 1024)[i % 4]) for i in range(57)]
    out = head + mid + tail
    assert len(out) == count and all(a[1] <= b[0] for a, b in zip(out, out[1:])) and out[-1][1] == N
    assert any(b < W < e for b, e in out)
    return out


def settings(i):
    """Every range its own lr, first step, betas and eps."""
    return dict(lr=1e-3 * (1 + i % 5), step=1 + (i * 7) % 11, beta1=(0.9, 0.8)[i % 2], beta2=(0.999, 0.99)[(i // 2) % 2],
                eps=(1e-8, 1e-6)[(i // 3) % 2])


def make_buffers(ranges, seed):
    """p, g, m, v on the device: a NaN bit pattern (one per buffer) wherever no range lies, data inside; every range holds a
    +0, a -0, a denormal and a tiny normal gradient among the random ones."""
    gen = torch.Generator().manual_seed(seed)
    bufs = {k: torch.full((N,), bits, dtype=torch.int32).view(torch.float32) for k, bits in NAN_BITS.items()}
    inside = torch.zeros(N, dtype=torch.bool)
    for b, e in ranges:
        n = e - b
        inside[b:e] = True
        bufs["p"][b:e] = torch.randn(n, generator=gen)
        bufs["g"][b:e] = torch.randn(n, generator=gen) * 3
        bufs["m"][b:e] = torch.randn(n, generator=gen) * 0.1
        bufs["v"][b:e] = torch.rand(n, generator=gen) * 0.01
        bufs["g"][b:b + 4] = torch.tensor([0.0, -0.0, 1e-40, 1e-30])
    return {k: t.to(DEV) for k, t in bufs.items()}, inside.to(DEV)


def bits(t):
    return t.view(torch.int32)


def expect_with_adam(want, ranges, segs, skip, grad_scale):
    """The parent's kernel on each zero-decay range of `want`, in place (every range starts 16-byte aligned)."""
    ops = _ops()
    for i, ((b, e), s) in enumerate(zip(ranges, segs)):
        if i not in skip:
            assert want["p"][b:e].data_ptr() % 16 == 0
            ops.adam(want["p"][b:e], want["g"][b:e], want["m"][b:e], want["v"][b:e], s["lr"], s["step"], s["beta1"],
                     s["beta2"], s["eps"], grad_scale)


def assert_same_bits(got, want, orig, inside, where, what):
    """all four buffers as int32: the ranges picked by `where` against the expected bits, the gaps against the NaN patterns
    they were filled with; the gradient is read-only everywhere"""
    for k in "pgmv":
        assert torch.equal(bits(got[k])[where], bits(want[k])[where]), f"{what}: {k} differs inside a segment"
        assert torch.equal(bits(got[k])[~inside], bits(orig[k])[~inside]), f"{what}: {k} written between segments"
        assert bool((bits(got[k])[~inside] == NAN_BITS[k]).all())
    assert torch.equal(bits(got["g"]), bits(orig["g"]))


# ----------------------------------------------------------------------------- zero decay: the bits of vqa_adam
@pytest.mark.parametrize("grad_scale", [1.0, 0.37])
@pytest.mark.parametrize("count", [1, 7, 64])
def test_zero_decay_segments_have_the_bits_of_vqa_adam(count, grad_scale):
    ops = _ops()
    ranges = layout(count)
    got, inside = make_buffers(ranges, 100 + count)
    orig = {k: t.clone() for k, t in got.items()}
    want = {k: t.clone() for k, t in got.items()}
    for k in range(3):                                             # three consecutive steps
        segs = [dict(begin=b, end=e, **settings(i)) for i, (b, e) in enumerate(ranges)]
        for s in segs:
            s["step"] += k
        ops.adam_segments(got["p"], got["g"], got["m"], got["v"], segs, grad_scale)
        expect_with_adam(want, ranges, segs, (), grad_scale)
        torch.cuda.synchronize()
        assert_same_bits(got, want, orig, inside, inside, f"{count} segments, step {k}")
    assert not torch.equal(bits(got["p"])[inside], bits(orig["p"])[inside])
    if count > 1:                                                  # the adjacent pairs really differ in lr and step
        assert settings(1)["lr"] != settings(2)["lr"] and settings(1)["step"] != settings(2)["step"]


# ----------------------------------------------------------------------------- decay: float64 torch, zero-decay neighbours exact
def tol_sum(n):
    return 4 * 2.0 ** -24 * math.sqrt(n)         # tests/test_streaming_gpu.py: the bound of its m and v checks


@pytest.mark.parametrize("grad_scale", [1.0, 0.37])
def test_decay_segments_follow_torch_and_their_neighbours_keep_the_bits_of_vqa_adam(grad_scale):
    ops = _ops()
    ranges = layout(7)
    decay = {1: (0.05, 0), 2: (0.1, 1), 4: (0.01, 1), 5: (0.2, 0)}          # range -> (weight_decay, decoupled); 0, 3, 6: none
    got, inside = make_buffers(ranges, 7)
    orig = {k: t.clone() for k, t in got.items()}
    want = {k: t.clone() for k, t in got.items()}
    plain = torch.zeros(N, dtype=torch.bool, device=DEV)
    for i, (b, e) in enumerate(ranges):
        plain[b:e] = i not in decay
    # float64 torch on the CPU, one optimiser per decaying range, scalars at their float32 values (streaming_ref.adam_ref)
    ref = {}
    for i, (wd, decoupled) in decay.items():
        b, e = ranges[i]
        s = settings(i)
        t = orig["p"][b:e].double().cpu().requires_grad_(True)
        t.grad = orig["g"][b:e].double().cpu() * A.f32(grad_scale)
        opt = (torch.optim.AdamW if decoupled else torch.optim.Adam)(
            [t], lr=A.f32(s["lr"]), betas=(A.f32(s["beta1"]), A.f32(s["beta2"])), eps=A.f32(s["eps"]), weight_decay=A.f32(wd))
        opt.state[t] = {"step": torch.tensor(0.0), "exp_avg": orig["m"][b:e].double().cpu(),
                        "exp_avg_sq": orig["v"][b:e].double().cpu()}
        ref[i] = (t, opt)
    worst = {"L2": 0.0, "decoupled": 0.0}
    for k in range(3):
        segs = []
        for i, (b, e) in enumerate(ranges):
            s = dict(begin=b, end=e, **settings(i))
            if i in decay:
                s.update(step=1, weight_decay=decay[i][0], decoupled=decay[i][1])      # torch counts from 1
            s["step"] += k
            segs.append(s)
        ops.adam_segments(got["p"], got["g"], got["m"], got["v"], segs, grad_scale)
        expect_with_adam(want, ranges, segs, decay, grad_scale)
        torch.cuda.synchronize()
        assert_same_bits(got, want, orig, inside, plain, f"decay layout, step {k}")
        for i, (t, opt) in ref.items():
            opt.step()
            b, e = ranges[i]
            kind = "decoupled" if decay[i][1] else "L2"
            name = f"adam_segments {kind} wd={decay[i][0]} grad_scale={grad_scale} step {k + 1} [{b}, {e})"
            err = A.check(f"{name} p", got["p"][b:e], t.detach())
            worst[kind] = max(worst[kind], err)
            A.check(f"{name} m", got["m"][b:e], opt.state[t]["exp_avg"], tol_sum(2 * 3))
            A.check(f"{name} v", got["v"][b:e], opt.state[t]["exp_avg_sq"], tol_sum(2 * 3))
    for kind, e in worst.items():
        print(f"[parity] adam_segments {kind} grad_scale={grad_scale} p, worst of 3 steps: max|err|/max|ref| = {e:.3e} (tol {A.ADAM_TOL:.1e})")


# ----------------------------------------------------------------------------- the two-phase recipe on tiny_plus
LR = 5e-4


def _fixture():
    g = Golden("tiny_plus")
    cfg = tiny_cfg(g.meta)
    return g, cfg, build(cfg, g.meta["V"], g.sd).eval()


def _snapshot(m, opt):
    opt._state()
    return {"p": m._flat_param.clone(), "m": opt.exp_avg.clone(), "v": opt.exp_avg_sq.clone()}


def _image_mask(m):
    lo, hi = m.group_range("image")
    mask = torch.zeros(m._flat_param.numel(), dtype=torch.bool, device=DEV)
    mask[lo:hi] = True
    return mask


def test_two_phase_recipe_freeze_then_unfreeze():
    from dl_vqa_amd.train import FusedAdam, run_batch, run_batch_features
    g, cfg, m = _fixture()
    _, _, legacy_model = _fixture()
    v, q, ql, a_idx, a_val = _bank_batch(g)
    bank_batch = (None, q, a_idx, a_val, g.t["a_len"][QSEL], torch.arange(7), ql)
    opt = FusedAdam(m, lr=LR, groups=[{"params": "image", "frozen": True}])
    legacy = FusedAdam(legacy_model, lr=LR)
    twin = A.TorchTwin(m, opt)
    names = [n for n, _ in m.named_parameters()]
    image_idx = [i for i, n in enumerate(names) if n.startswith("image.")]
    start = _snapshot(m, opt)
    image = _image_mask(m)
    # phase 1: two steps on a feature bank (each model its own: a bank belongs to the model that encoded it)
    banks = {id(model): _encode(model, v, with_vprime=False) for model in (m, legacy_model)}
    for it in range(2):
        for model, o in ((m, opt), (legacy_model, legacy)):
            loss, _ = run_batch_features(model, bank_batch, 12, banks[id(model)], BANK_INDEX)
            o.zero_grad()
            loss.backward()
            if o is opt:
                twin.step(m, opt)
            o.step()
        torch.cuda.synchronize()
        now = _snapshot(m, opt)
        for k in "pmv":                                            # image.*: value and moments keep their bits
            assert torch.equal(bits(now[k])[image], bits(start[k])[image]), (it, k)
        assert float(now["m"][image].abs().max()) == 0.0 and float(now["v"][image].abs().max()) == 0.0
        sd = opt.state_dict()
        assert not any(i in sd["state"] for i in image_idx) and len(sd["state"]) == len(names) - len(image_idx)
        assert all(float(st["step"]) == it + 1 for st in sd["state"].values())
        # the trained parameters: the legacy optimiser's bits (same arithmetic, and a global step equals a per-parameter
        # step for parameters that are never skipped)
        assert torch.equal(bits(m._flat_param), bits(legacy_model._flat_param)), it
        assert torch.equal(bits(opt.exp_avg), bits(legacy.exp_avg)) and torch.equal(bits(opt.exp_avg_sq), bits(legacy.exp_avg_sq))
        assert not torch.equal(bits(now["p"])[~image], bits(start["p"])[~image])
        for n, p in m.named_parameters():
            A.check(f"phase 1 step {it + 1} {n}", p.data, twin.params[n].data)
    # phase 2: the encoder joins
    opt.unfreeze("image")
    full_batch = (g.t["v"], g.t["q"], g.t["a_idx"], g.t["a_val"], g.t["a_len"], torch.arange(g.t["q"].shape[0]), g.t["q_len"])
    for it in range(2):
        loss, _ = run_batch(m, None, full_batch, 12)
        opt.zero_grad()
        loss.backward()
        twin.step(m, opt)
        opt.step()
        torch.cuda.synchronize()
        for n, p in m.named_parameters():
            A.check(f"phase 2 step {it + 1} {n}", p.data, twin.params[n].data)
        sd = opt.state_dict()
        steps = {i: int(float(st["step"])) for i, st in sd["state"].items()}
        assert steps == twin.steps()
        assert all(steps[i] == (it + 1 if i in image_idx else it + 3) for i in range(len(names)))
    assert not torch.equal(bits(m._flat_param)[image], bits(start["p"])[image])


def test_lr_scale_of_one_group_is_vqa_adam_with_the_scaled_rate():
    from dl_vqa_amd.train import FusedAdam, run_batch
    ops = _ops()
    g, cfg, m = _fixture()
    full_batch = (g.t["v"], g.t["q"], g.t["a_idx"], g.t["a_val"], g.t["a_len"], torch.arange(g.t["q"].shape[0]), g.t["q_len"])
    opt = FusedAdam(m, lr=LR, groups=[{"params": "image", "lr_scale": 0.1}])
    loss, _ = run_batch(m, None, full_batch, 12)
    opt.zero_grad()
    loss.backward()
    assert all(p.grad is not None for p in m.parameters())
    opt._state()
    before = {"p": m._flat_param.clone(), "g": m._flat_grad.clone(), "m": opt.exp_avg.clone(), "v": opt.exp_avg_sq.clone()}
    n = m._flat_param.numel()
    lo, hi = m.group_range("image")
    assert lo % 4 == 0 and hi % 4 == 0 and 0 < hi - lo < n

    def with_adam(image_lr):
        w = {k: t.clone() for k, t in before.items()}
        for b, e, lr in ((0, lo, LR), (lo, hi, image_lr), (hi, n, LR)):
            if e > b:
                ops.adam(w["p"][b:e], w["g"][b:e], w["m"][b:e], w["v"][b:e], lr, 1)
        return w
    want = with_adam(LR * 0.1)                    # the product in double, rounded to float32 by the call: what step() passes
    full = with_adam(LR)
    opt.step()
    torch.cuda.synchronize()
    assert torch.equal(bits(m._flat_param), bits(want["p"]))
    assert torch.equal(bits(opt.exp_avg), bits(want["m"])) and torch.equal(bits(opt.exp_avg_sq), bits(want["v"]))
    assert not torch.equal(bits(m._flat_param)[lo:hi], bits(full["p"])[lo:hi])         # the scale reaches the image range ...
    rest = ~_image_mask(m)
    assert torch.equal(bits(m._flat_param)[rest], bits(full["p"])[rest])               # ... and nothing else
    assert [g["lr"] for g in opt.param_groups] == [LR, LR] and opt.param_groups[0]["lr_scale"] == 0.1
