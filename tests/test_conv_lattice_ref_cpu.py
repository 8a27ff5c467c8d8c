"""The lattice inputs and the closed-form reference of tests/conv_lattice_ref.py, checked without a GPU for every case of
tests/test_conv_lattice_gpu.py: the closed form equals float64 autograd bit for bit, every operand and every sum is exact in
the formats the kernels use, ties and exact zeros are frequent enough, and the two faults the GPU file exists to catch --
`>=` for `>` among a window's candidates, `>= 0` for `> 0` in the aliveness test -- change the reference's bytes, dbias and dX."""
import pytest
import torch
import torch.nn.functional as F

from tests import conv_lattice_ref as L

KEYS = L.all_keys()
_id = lambda k: "B{}_Ci{}_{}x{}_Co{}_k{}_s{}".format(*k)


def test_the_case_list_has_a_5x5_and_a_2x2_stride_2_case():
    assert any(k[5] == 5 for k in KEYS) and any(k[5] == 2 and k[6] == 2 for k in KEYS) and any(k[6] == 2 and k[5] == 3 for k in KEYS)


@pytest.mark.parametrize("k", KEYS, ids=_id)
def test_closed_form_equals_float64_autograd(k):
    case, ref = L.cached(*k)
    x, w, b = (t.clone().requires_grad_(True) for t in (case.x, case.w, case.b))
    y = F.max_pool2d(torch.relu(F.conv2d(x, w, b, stride=case.stride)), 2, 2)
    y.backward(case.dy)
    assert torch.equal(ref.pooled, y.detach())
    assert torch.equal(ref.dx, x.grad) and torch.equal(ref.dw, w.grad) and torch.equal(ref.db, b.grad)
    assert ref.argmax.dtype == torch.uint8 and ref.argmax.shape == case.dy.shape
    assert torch.equal(ref.argmax == 4, ref.pooled == 0)


@pytest.mark.parametrize("k", KEYS, ids=_id)
def test_every_operand_and_every_sum_is_exact(k):
    case, ref = L.cached(*k)
    L.assert_exact(case)
    for t in (case.x, case.w, case.b, case.dy, ref.z, ref.pooled, ref.dx, ref.dw, ref.db):
        assert torch.equal(t.float().double(), t)
    if k in L.bf16_keys():
        for t in (case.x, case.w, case.dy):                     # the bias stays fp32 in every family
            assert torch.equal(t.to(torch.bfloat16).double(), t)
        assert torch.equal(case.x.half().double(), case.x)      # the first block's fp16 image


def test_assert_exact_refuses_a_case_over_budget_or_off_the_lattice():
    case, _ = L.cached(*KEYS[0])
    with pytest.raises(AssertionError):
        L.assert_exact(case._replace(x=case.x * 2.0 ** 21))
    with pytest.raises(AssertionError):
        L.assert_exact(case._replace(w=case.w + 0.25))


@pytest.mark.parametrize("k", KEYS, ids=_id)
def test_ties_and_exact_zeros_are_frequent(k):
    case, _ = L.cached(*k)
    s = L.tie_stats(case)
    n = s["windows"]
    print(f"[lattice-ref] {_id(k)}: windows {n} tied {s['tied']:.3f} zero-max {s['zero_max']:.4f} dead {s['dead']:.2f} "
          f"first-max != 0 {s['first_nonzero']:.2f} later tie {s['later_tie']:.2f} max|z| {s['max_abs_z']}")
    assert s["tied"] >= 0.03 and s["tied"] * n >= 100
    assert s["first_nonzero"] >= 0.25 and s["later_tie"] >= 0.25
    assert s["zero_max"] >= 0.005 and s["zero_max"] * n >= 50
    assert s["dead"] >= 0.10 and s["alive"] >= 0.50


@pytest.mark.parametrize("mutant", ["tie_ge", "alive_ge"])
@pytest.mark.parametrize("k", KEYS, ids=_id)
def test_the_reference_tells_the_mutants_apart(k, mutant):
    """The bias gradient sums a window's dy whichever of its pixels receives it, so the tie mutant cannot move dbias (it is
    asserted to be unchanged); it moves the bytes, dX and dW.  The aliveness mutant moves all four."""
    case, ref = L.cached(*k)
    bad = L.reference(*case, **{mutant: True})
    assert not torch.equal(bad.argmax, ref.argmax)
    assert not torch.equal(bad.dx, ref.dx) and not torch.equal(bad.dw, ref.dw)
    assert torch.equal(bad.db, ref.db) == (mutant == "tie_ge")
    assert torch.equal(bad.pooled, ref.pooled)                  # neither fault shows in the forward values


def test_layout_helpers_round_trip():
    g = torch.Generator().manual_seed(0)
    t = torch.randint(-4, 5, (2, 3, 5, 7), generator=g).double()
    p = L.nhwc(t, 4)
    assert p.shape == (2, 5, 7, 4) and torch.equal(L.nchw(p)[:, :3], t) and float(p[..., 3].abs().max()) == 0.0
    a = torch.randint(0, 5, (2, 4, 6, 32), generator=g).to(torch.uint8)
    c = L.to_c16(a)
    assert c.shape == (2, 2, 4, 6, 16) and torch.equal(L.from_c16(c), a) and torch.equal(c[1, 1, 2, 3], a[1, 2, 3, 16:])
    v = torch.randn(3, 8, generator=g).double().float().double()
    hi = v.to(torch.bfloat16)
    mid = (v - hi.double()).to(torch.bfloat16)
    lo = (v - hi.double() - mid.double()).to(torch.bfloat16)
    packed = torch.stack([hi.view(3, 2, 4), mid.view(3, 2, 4), lo.view(3, 2, 4)], dim=2)     # [3, C/4, 3, 4]
    assert torch.equal(L.x3_unpack(packed), v)
    assert L.rne_bf16(torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8], dtype=torch.float64)).tolist() == [1.0, 1.015625]
    assert L.rne_fp16(torch.tensor([2049.0, 2051.0], dtype=torch.float64)).tolist() == [2048.0, 2052.0]
    with pytest.raises(AssertionError):
        L.rne_bf16(torch.tensor([1.0 + 2.0 ** -30], dtype=torch.float64))
