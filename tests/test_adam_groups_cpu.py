"""CPU: FusedAdam's parameter groups and the argument checks of vqa_adam_segments.

No kernel runs here.  The model is the CPU stand-in of tests/test_autograd_glue_cpu.py and ops.adam_segments is replaced by
the float64 restatement of the table (tests/adam_groups_ref.py), so what is under test is the host logic: which ranges the
table lists, which parameters' steps advance, what state_dict() says, and that torch.optim.Adam agrees step for step.
"""
import ctypes
import os
import re

import pytest
import torch

from tests import adam_groups_ref as A
from tests.test_autograd_glue_cpu import make_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR = 1e-2


# ----------------------------------------------------------------------------- binding and argument checks
def test_symbol_is_declared_bound_and_exported():
    from dl_vqa_amd import _lib, build
    build.build_library(verbose=False)
    lib = _lib.load()
    text = open(os.path.join(ROOT, "include", "vqa_hip.h")).read()
    head = text[:re.search(r"^#define\s+VQA_ABI_VERSION", text, flags=re.M).start()]
    assert "vqa_adam_segments" in head                      # listed with the other append-only additions
    assert _lib.header_abi_version() == 9
    assert "vqa_adam_segments" in _lib.PROTOTYPES and hasattr(lib, "vqa_adam_segments")
    assert ctypes.sizeof(_lib.AdamSegment) == 48            # two int64, five floats, two ints, padded to 8 bytes
    assert int(re.search(r"^#define\s+VQA_ADAM_MAX_SEGMENTS\s+(\d+)", text, flags=re.M).group(1)) == _lib.ADAM_MAX_SEGMENTS == 64


def _call(segments, n=4096, n_segs=None, ptrs=(4096, 8192, 12288, 16384)):
    """vqa_adam_segments with made-up device pointers: every check below returns before a HIP call."""
    from dl_vqa_amd import _lib, ops
    lib = _lib.load()
    table = ops.adam_segment_table(segments)
    rc = lib.vqa_adam_segments(*ptrs, n, table, len(table) if n_segs is None else n_segs, 1.0, None)
    return rc, lib.vqa_last_error()


def test_argument_validation_without_gpu():
    ok = (0, 64, 1e-3)
    seg = lambda b, e, **kw: dict(begin=b, end=e, lr=1e-3, **kw)
    for what, (rc, err) in {
        "n_segs": _call([ok], n_segs=0),
        "n_segs ": _call([seg(4 * i, 4 * i + 4) for i in range(65)]),
        "overlaps": _call([seg(0, 64), seg(60, 128)]),
        "overlaps ": _call([seg(64, 128), seg(0, 64)]),                     # unsorted
        "out of range": _call([seg(0, 64), seg(4032, 4100)]),               # end past n
        "out of range ": _call([seg(64, 64)]),                              # empty
        "out of range  ": _call([seg(-4, 64)]),
        "aligned to 4": _call([seg(2, 64)]),
        "aligned to 4 ": _call([seg(0, 63)]),
        "step=0": _call([seg(0, 64, step=0)]),
        "weight_decay": _call([seg(0, 64, weight_decay=-0.1)]),
        "16-byte aligned": _call([ok], ptrs=(4096, 8192 + 8, 12288, 16384)),
        "null pointer": _call([ok], ptrs=(4096, 8192, None, 16384)),
    }.items():
        assert rc == 1 and what.strip().encode() in err, (what, rc, err)
    from dl_vqa_amd import _lib
    lib = _lib.load()
    assert lib.vqa_adam_segments(4096, 8192, 12288, 16384, 4096, None, 1, 1.0, None) == 1 and b"null pointer" in lib.vqa_last_error()


def test_segment_table_from_tuples_and_dicts():
    from dl_vqa_amd import ops
    t = ops.adam_segment_table([(0, 64, 1e-3), dict(begin=64, end=128, lr=2e-3, step=7, weight_decay=0.5, decoupled=True)])
    assert (t[0].begin, t[0].end, t[0].step, t[0].decoupled, t[0].weight_decay) == (0, 64, 1, 0, 0.0)
    assert (t[1].begin, t[1].end, t[1].step, t[1].decoupled, t[1].weight_decay) == (64, 128, 7, 1, 0.5)
    assert t[0].beta1 == A.f32(0.9) and t[1].lr == A.f32(2e-3)
    with pytest.raises(ValueError):
        ops.adam_segment_table([dict(begin=0, end=64, lr=1e-3, amsgrad=True)])
    with pytest.raises(ValueError):
        ops.adam_segment_table([dict(begin=0, end=64)])


# ----------------------------------------------------------------------------- host logic on the stand-in model
@pytest.fixture
def table_calls(monkeypatch):
    """ops.adam_segments replaced by the float64 table; every call's segment list is recorded."""
    from dl_vqa_amd import ops
    calls = []

    def cpu_table(p, g, m, v, segments, grad_scale=1.0):
        calls.append([tuple(s) for s in segments])
        A.adam_segments_f64(p, g, m, v, segments, grad_scale)
    monkeypatch.setattr(ops, "adam_segments", cpu_table)
    return calls


def give_grads(model, seed, skip=()):
    """The same made-up gradient for every parameter (outside the flat buffer: step() copies it into its slot)."""
    g = torch.Generator().manual_seed(seed)
    for n, p in model.named_parameters():
        p.grad = None if n in skip else torch.randn(p.shape, generator=g)


def ceil64(k):
    return (k + 63) // 64 * 64


def snapshot(model, opt):
    opt._state()
    return model._flat_param.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone()


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_segments_cover_the_updated_slots_and_merge(table_calls):
    from dl_vqa_amd.train import FusedAdam
    m, _ = make_model()
    opt = FusedAdam(m, lr=LR, groups=[{"params": "image", "frozen": True},
                                      {"params": ["attention", "classifier.lin2.bias"], "lr_scale": 0.5, "weight_decay": 0.01}])
    assert [g["spec"] for g in opt.param_groups] == [("image",), ("attention", "classifier.lin2.bias"), ()]
    no_grad = "text.embedding.weight"
    give_grads(m, 1, skip=(no_grad,))
    before = snapshot(m, opt)
    opt.step()
    (segments,) = table_calls
    _, _, offsets = m.flat_buffers()
    group_of = {n: k for k, g in enumerate(opt.param_groups) for n in g["params"]}
    # exactly the padded slots of the updated parameters, each inside a segment with its own group's settings
    covered = torch.zeros(m._flat_param.numel(), dtype=torch.bool)
    for s in segments:
        assert not covered[s[0]:s[1]].any() and s[0] % 4 == 0 and s[1] % 4 == 0
        covered[s[0]:s[1]] = True
    expect = torch.zeros_like(covered)
    for n, (o, k) in offsets.items():
        if group_of[n] != 0 and n != no_grad:
            expect[o:o + ceil64(k)] = True
            g = opt.param_groups[group_of[n]]
            (s,) = [s for s in segments if s[0] <= o and o + ceil64(k) <= s[1]]
            assert s[2:] == (LR * g["lr_scale"], 0.9, 0.999, 1e-8, g["weight_decay"], 1, 0), n
    assert torch.equal(covered, expect)
    assert list(segments) == sorted(segments)
    for a, b in zip(segments, segments[1:]):                       # merged: touching neighbours differ in their settings
        assert a[1] < b[0] or a[2:] != b[2:]
    assert len(segments) < sum(1 for n in offsets if group_of[n] != 0 and n != no_grad)      # and something was merged
    # the frozen group and the grad-less parameter keep value and moments, bit for bit, and have no state
    after = snapshot(m, opt)
    for was, now in zip(before, after):
        assert same_bits(was[~expect], now[~expect])
    assert not same_bits(before[0][expect], after[0][expect])
    names = [n for n, _ in m.named_parameters()]
    sd = opt.state_dict()
    assert sorted(sd["state"]) == [i for i, n in enumerate(names) if group_of[n] != 0 and n != no_grad]
    assert all(opt.steps[n] == 0 for n in opt.param_groups[0]["params"]) and opt.steps[no_grad] == 0


def test_double_match_and_empty_match_raise():
    from dl_vqa_amd.train import FusedAdam
    m, _ = make_model()
    with pytest.raises(ValueError, match="matched by group 0 and by group 1"):
        FusedAdam(m, lr=LR, groups=[{"params": "text"}, {"params": "text.embedding"}])
    with pytest.raises(ValueError, match="matches no parameter"):
        FusedAdam(m, lr=LR, groups=[{"params": ["image", "imag"]}])
    with pytest.raises(ValueError, match="may set"):
        FusedAdam(m, lr=LR, groups=[{"params": "image", "amsgrad": True}])
    opt = FusedAdam(m, lr=LR, groups=[{"params": "image"}])
    with pytest.raises(ValueError, match="no group was built"):
        opt.unfreeze("text")
    with pytest.raises(RuntimeError, match="needs parameter groups"):
        FusedAdam(m, lr=LR).freeze("image")


def test_nothing_to_update_raises(table_calls):
    from dl_vqa_amd.train import FusedAdam
    m, _ = make_model()
    opt = FusedAdam(m, lr=LR, groups=[{"params": "image", "frozen": True}])
    with pytest.raises(RuntimeError, match="no parameter has a gradient"):
        opt.step()
    give_grads(m, 1, skip=[n for n, _ in m.named_parameters() if not n.startswith("image.")])
    with pytest.raises(RuntimeError, match="no parameter has a gradient"):
        opt.step()
    assert not table_calls and not any(opt.steps.values())


def test_more_than_64_segments_raise(table_calls):
    from dl_vqa_amd import train
    m, _ = make_model()
    names = [n for n, _ in m.named_parameters()]
    opt = train.FusedAdam(m, lr=LR, groups=[{"params": n, "lr_scale": 1.0 + i} for i, n in enumerate(names[:6])])
    give_grads(m, 1)
    old, train.MAX_ADAM_SEGMENTS = train.MAX_ADAM_SEGMENTS, 3
    try:
        with pytest.raises(RuntimeError, match="one launch"):
            opt.step()
    finally:
        train.MAX_ADAM_SEGMENTS = old
    assert not table_calls and not any(opt.steps.values())
    opt.step()
    assert len(table_calls) == 1 and all(v == 1 for v in opt.steps.values())


# ----------------------------------------------------------------------------- freeze -> unfreeze against torch
def test_freeze_then_unfreeze_follows_torch_step_for_step(table_calls):
    from dl_vqa_amd.train import FusedAdam
    m, _ = make_model()
    opt = FusedAdam(m, lr=LR, groups=[{"params": "image", "frozen": True, "lr_scale": 0.3},
                                      {"params": "text.embedding", "weight_decay": 0.05},
                                      {"params": "classifier", "betas": (0.8, 0.99), "eps": 1e-6}])
    twin = A.TorchTwin(m, opt)
    names = [n for n, _ in m.named_parameters()]
    image = [i for i, n in enumerate(names) if n.startswith("image.")]
    for it in range(7):
        if it == 3:
            opt.unfreeze("image")
        if it == 5:
            opt.param_groups[1]["frozen"] = True                   # setting the flag directly works as well
        give_grads(m, 10 + it, skip=("attention.x_conv.bias",) if it == 4 else ())
        scale = 0.37 if it == 2 else 1.0
        opt.step(grad_scale=scale)
        twin.step(m, opt, grad_scale=scale)
        for n, p in m.named_parameters():
            A.check(f"step {it} {n}", p.data, twin.params[n].data)
        sd = opt.state_dict()
        mine = {i: int(float(st["step"])) for i, st in sd["state"].items()}
        assert mine == twin.steps(), it                            # the same entries with the same steps, none extra
        assert all((i in mine) == (it >= 3) for i in image)
    assert {mine[i] for i in image} == {4}
    assert mine[names.index("classifier.lin2.weight")] == 7 and mine[names.index("attention.x_conv.bias")] == 6
    assert mine[names.index("text.embedding.weight")] == 5


def test_decoupled_decay_follows_adamw(table_calls):
    from dl_vqa_amd.train import FusedAdam
    m, _ = make_model()
    names = [n for n, _ in m.named_parameters()]
    opt = FusedAdam(m, lr=LR, groups=[{"params": [n for n in names if n.endswith("weight")], "weight_decay": 0.1, "decoupled": True},
                                      {"params": [n for n in names if not n.endswith("weight")], "weight_decay": 0.02,
                                       "decoupled": True, "lr_scale": 2.0}])
    twin = A.TorchTwin(m, opt)
    assert isinstance(twin.opt, torch.optim.AdamW)
    for it in range(3):
        give_grads(m, 20 + it)
        opt.step()
        twin.step(m, opt)
        for n, p in m.named_parameters():
            A.check(f"step {it} {n}", p.data, twin.params[n].data)


# ----------------------------------------------------------------------------- state_dict interchange
GROUPS = [{"params": "image", "frozen": True}, {"params": "text", "weight_decay": 0.05, "lr_scale": 0.5},
          {"params": "attention", "betas": (0.8, 0.99)}]


def _trained(table_calls, seed=3):
    from dl_vqa_amd.train import FusedAdam
    m, _ = make_model(seed)
    opt = FusedAdam(m, lr=LR, groups=GROUPS)
    for it in range(2):
        give_grads(m, 30 + it)
        opt.step()
    opt.unfreeze("image")
    give_grads(m, 32)
    opt.step()
    return m, opt


def test_state_dict_round_trip(table_calls):
    from dl_vqa_amd.train import FusedAdam
    m, opt = _trained(table_calls)
    sd = opt.state_dict()
    names = [n for n, _ in m.named_parameters()]
    assert [g["params"] for g in sd["param_groups"]] == [[names.index(n) for n in g["params"]] for g in opt.param_groups]
    assert sorted(i for g in sd["param_groups"] for i in g["params"]) == list(range(len(names)))
    assert [(g["lr_scale"], g["frozen"], g["decoupled"], g["weight_decay"]) for g in sd["param_groups"]] == \
        [(1.0, False, False, 0.0), (0.5, False, False, 0.05), (1.0, False, False, 0.0), (1.0, False, False, 0.0)]
    m2, _ = make_model(3)
    m2.load_state_dict(m.state_dict())
    opt2 = FusedAdam(m2, lr=123.0, groups=[dict(g, frozen=True) for g in GROUPS])     # everything the dict carries is restored
    opt2.load_state_dict(sd)
    assert opt2.steps == opt.steps and {opt.steps[n] for n in names if n.startswith("image.")} == {1}
    sd2 = opt2.state_dict()
    assert sd2["param_groups"] == sd["param_groups"] and sorted(sd2["state"]) == sorted(sd["state"])
    for i, st in sd["state"].items():
        assert float(sd2["state"][i]["step"]) == float(st["step"])
        assert same_bits(sd2["state"][i]["exp_avg"], st["exp_avg"]) and same_bits(sd2["state"][i]["exp_avg_sq"], st["exp_avg_sq"])
    for o, mdl in ((opt, m), (opt2, m2)):                         # and both make the same next step
        give_grads(mdl, 40)
        o.step()
    assert same_bits(m._flat_param, m2._flat_param) and table_calls[-1] == table_calls[-2]
    with pytest.raises(ValueError, match="groups"):
        FusedAdam(m2, lr=LR, groups=GROUPS[:1]).load_state_dict(sd)


def test_torch_adam_loads_the_state_dict_and_makes_the_same_next_step(table_calls):
    m, opt = _trained(table_calls)
    sd = opt.state_dict()
    params = {n: p.detach().double().clone().requires_grad_(True) for n, p in m.named_parameters()}
    tor = torch.optim.Adam([{"params": [params[n] for n in g["params"]]} for g in opt.param_groups], lr=1.0)
    tor.load_state_dict(sd)
    for tg, g in zip(tor.param_groups, opt.param_groups):
        assert (tg["lr"], tuple(tg["betas"]), tg["eps"], tg["weight_decay"]) == (g["lr"], g["betas"], g["eps"], g["weight_decay"])
        assert (tg["lr_scale"], tg["frozen"], tg["decoupled"]) == (g["lr_scale"], g["frozen"], g["decoupled"])     # ride along
        tg["lr"] = g["lr"] * g["lr_scale"]                        # torch knows no lr_scale: the documented hand-over
    give_grads(m, 41)
    for n, p in m.named_parameters():
        params[n].grad = p.grad.double()
    opt.step()
    tor.step()
    for n, p in m.named_parameters():
        A.check(n, p.data, params[n].data)
        assert int(float(tor.state[params[n]]["step"])) == opt.steps[n]


# ----------------------------------------------------------------------------- schedule, legacy constructor
def test_update_learning_rate_writes_every_group_and_keeps_the_ratio(table_calls):
    from dl_vqa_amd.train import FusedAdam, update_learning_rate
    m, _ = make_model()
    opt = FusedAdam(m, lr=LR, groups=[{"params": "image", "lr_scale": 0.1}, {"params": "text", "lr_scale": 3.0}])
    update_learning_rate(opt, 25000, LR)
    lr = LR * 0.5 ** 0.5
    assert [g["lr"] for g in opt.param_groups] == [lr, lr, lr]
    give_grads(m, 1)
    opt.step()
    rates = {s[2] for s in table_calls[-1]}
    assert rates == {lr * 0.1, lr * 3.0, lr}


def test_legacy_constructor_never_reaches_the_segment_kernel(monkeypatch):
    from dl_vqa_amd import ops
    from dl_vqa_amd.train import FusedAdam
    from oracle import vqa_oracle as O
    calls = []

    def cpu_adam(p, g, m1, m2, lr, step, b1, b2, eps, grad_scale=1.0):
        calls.append(step)
        O.adam_step(p, g * grad_scale, m1, m2, step, lr, b1, b2, eps)

    def never(*a, **k):
        raise AssertionError("FusedAdam without groups called ops.adam_segments")
    monkeypatch.setattr(ops, "adam", cpu_adam)
    monkeypatch.setattr(ops, "adam_segments", never)
    m, _ = make_model()
    opt = FusedAdam(m, lr=LR)
    assert opt.param_groups == [{"lr": LR, "betas": (0.9, 0.999), "eps": 1e-8}]
    for it in range(2):
        give_grads(m, 50 + it, skip=("text.embedding.weight",))
        opt.step()
    assert calls == [1, 2]
    sd = opt.state_dict()
    assert len(sd["param_groups"]) == 1 and len(sd["state"]) == len(list(m.parameters()))      # the legacy format, unchanged
    opt.load_state_dict(sd)
    assert opt.step_count == 2
