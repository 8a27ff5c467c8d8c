"""The lattice inputs and the closed-form reference of tests/conv_lattice_ref.py, checked without a GPU for every case of
tests/test_conv_lattice_gpu.py: the closed form equals float64 autograd bit for bit, every operand and every sum is exact in
the formats the kernels use, ties and exact zeros are frequent enough, and the two faults the GPU file exists to catch --
`>=` for `>` among a window's candidates, `>= 0` for `> 0` in the aliveness test -- change the reference's bytes, dbias and dX."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests import conv_lattice_ref as L
from tests import gemm_lattice_ref as G

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


# ------------------------------------------------------------------------------------------------ plane lattices (fp32x3)
# The cases of tests/test_conv_lattice_gpu.py whose mid and lo planes are not zero (conv_lattice_ref.PLANE_LATTICES).
PLANE_KEYS = L.plane_keys()
_pid = lambda lk: f"{lk[0]}_" + _id(lk[1])
OPERAND = {"xi": "x", "wi": "w", "dyi": "dy"}           # the operand the table calls "three planes"


def _plane(lk):
    return L.cached(*lk[1], lattice=lk[0])


def _compared(ref, which):
    """what the GPU file compares for a pass"""
    return {"forward": (ref.pooled, ref.argmax), "dX": (ref.dx,), "dW": (ref.dw,)}[which]


@pytest.mark.parametrize("lk", PLANE_KEYS, ids=_pid)
def test_plane_cases_are_exact(lk):
    case, ref = _plane(lk)
    budgets = L.assert_exact_planes(case, ref.argmax)
    print(f"[lattice-ref] {_pid(lk)}: " + " ".join(f"{n} {v / L.LIMIT_X3:.3f}" for n, v in budgets.items()) + " of 2^24")
    for t in (case.x, case.w, case.b, case.dy, ref.z, ref.pooled, ref.dx, ref.dw, ref.db):
        assert torch.equal(t.float().double(), t)
    assert float(case.b.abs().max()) <= 4
    with pytest.raises(AssertionError):                         # the 2^22 condition of the bf16-exact cases is untouched
        L.assert_exact(case)


@pytest.mark.parametrize("lk", PLANE_KEYS, ids=_pid)
def test_plane_closed_form_equals_float64_autograd(lk):
    case, ref = _plane(lk)
    x, w, b = (t.clone().requires_grad_(True) for t in (case.x, case.w, case.b))
    y = F.max_pool2d(torch.relu(F.conv2d(x, w, b, stride=case.stride)), 2, 2)
    y.backward(case.dy)
    assert torch.equal(ref.pooled, y.detach())
    assert torch.equal(ref.dx, x.grad) and torch.equal(ref.dw, w.grad) and torch.equal(ref.db, b.grad)
    assert torch.equal(ref.argmax == 4, ref.pooled == 0)


def test_plane_conditions_that_must_fail_do_fail():
    B, Ci, H, W, Co, ks, stride = L.key(*L.PLANE_SHAPES[0])
    g = torch.Generator().manual_seed(1)
    xi, _ = L.cached(B, Ci, H, W, Co, ks, stride, lattice="xi")
    L.assert_exact_planes(xi)
    with pytest.raises(AssertionError, match="forward: sum"):                   # a dense w under xi
        L.assert_exact_planes(xi._replace(w=L._small(g, xi.w.shape)))
    with pytest.raises(AssertionError, match="off the lattice"):
        L.assert_exact_planes(xi._replace(w=xi.w * 0.5))
    dense_dy = L.plane_case("iii", B, Ci, H, W, Co, stride, seed=H, iii_dy=9 * Co)       # a dy that is not thinned under iii
    with pytest.raises(AssertionError, match="dW: sum"):
        L.assert_exact_planes(dense_dy)
    # both operands with three planes: the dropped products are not zero
    wi, _ = L.cached(B, Ci, H, W, Co, ks, stride, lattice="wi")
    with pytest.raises(AssertionError, match="dropped plane product"):
        L.assert_exact_planes(xi._replace(w=wi.w))


def test_the_naive_plane_scales_leave_the_lo_plane_empty():
    """2^16 : 2^8 : 1 under the round-to-nearest-even split: 65536 + 256 + 1 is 66048 - 255, two planes.  The digits of
    tests/gemm_lattice_ref.py are the planes."""
    g = torch.Generator().manual_seed(0)
    h, m, l = G._digits(g, (4096,), True), G._digits(g, (4096,), True), G._digits(g, (4096,))
    naive = 2.0 ** 16 * h + 2.0 ** 8 * m + l
    assert float(G.x3_planes(naive)[2].abs().max()) == 0.0 and L.plane_occupancy(naive)["all"] == 0.0
    good = 3 * 2.0 ** 17 * h + 3 * 2.0 ** 8 * m + l
    ph, pm, pl = G.x3_planes(good)
    assert torch.equal(ph, 3 * 2.0 ** 17 * h) and torch.equal(pm, 3 * 2.0 ** 8 * m) and torch.equal(pl, l)


@pytest.mark.parametrize("lk", PLANE_KEYS, ids=_pid)
def test_plane_occupancy(lk):
    """measured with x3_planes, not with the generator's digits"""
    case, _ = _plane(lk)
    occ = {n: L.plane_occupancy(getattr(case, n)) for n in ("x", "w", "dy")}
    print(f"[lattice-ref] {_pid(lk)}: " + " ".join(f"{n} hi {o['hi']:.2f} mid {o['mid']:.2f} lo {o['lo']:.2f}" for n, o in occ.items()))
    if lk[0] == "iii":                       # the image; w and dy are thinned for the budgets (w to 150 in 9 Ci)
        assert occ["x"]["hi"] >= 0.25 and occ["x"]["mid"] >= 0.25
        for o in occ.values():
            assert o["mid"] >= 0.5 * o["hi"] > 0 and o["lo"] == 0
    else:
        assert occ[OPERAND[lk[0]]]["all"] >= 0.5
        for n in set(occ) - {OPERAND[lk[0]]}:
            assert occ[n]["mid"] == 0 and occ[n]["lo"] == 0 and occ[n]["hi"] > 0


@pytest.mark.parametrize("lk", PLANE_KEYS, ids=_pid)
def test_plane_reach(lk):
    """no row of a contraction is all zeros on either side: every k of the forward and of dX, every 32-pixel K-step of dW"""
    case, ref = _plane(lk)
    for which in L.PASSES:
        rows, empty = L.empty_rows(case, ref.argmax, which)
        assert rows > 0 and empty == 0, (which, rows, empty)
    Ho, Wo, Hp, Wp = L.out_hw(case.x.shape[2], case.x.shape[3], 3, case.stride)
    assert L.empty_rows(case, ref.argmax, "forward")[0] == 9 * case.x.shape[1]
    assert L.empty_rows(case, ref.argmax, "dX")[0] == 9 * case.w.shape[0]
    assert L.empty_rows(case, ref.argmax, "dW")[0] == -(-case.x.shape[0] * 4 * Hp * Wp // 32)


@functools.lru_cache(maxsize=None)
def _shares(lk, which):
    """{pair: (elements of the compared tensors that change when the pair is left out, their number)}; asserts on the way that
    the six kept pairs together are the reference"""
    case, ref = _plane(lk)
    terms = L.pair_terms(case, ref.argmax, which)
    want = _compared(ref, which)
    full = L.pass_by_pairs(case, ref.argmax, which, L.PAIRS, terms)
    assert len(full) == len(want) and all(torch.equal(a, b) for a, b in zip(full, want)), (lk, which)
    out = {}
    for p in L.PAIRS:
        mutant = L.pass_by_pairs(case, ref.argmax, which, [q for q in L.PAIRS if q != p], terms)
        out[p] = (sum(int((a != b).sum()) for a, b in zip(mutant, want)), sum(a.numel() for a in want))
    return out


@pytest.mark.parametrize("lk", PLANE_KEYS, ids=_pid)
def test_six_plane_pairs_are_the_reference(lk):
    for which in L.PASSES:
        _shares(lk, which)


@pytest.mark.parametrize("pair", L.PAIRS)
@pytest.mark.parametrize("which", L.PASSES)
def test_a_dropped_plane_pair_shows(which, pair):
    """The MUTANT kernel that leaves one of the six kept products out of a pass: some plane case of tests/test_conv_lattice_gpu.py
    must differ from it in at least 10 % of the elements compared for that pass (pooled and bytes; dX; dW), and in at least
    1 000.  A condition on the inputs: a case that misses it needs other inputs, not another bound."""
    best = max(PLANE_KEYS, key=lambda lk: _shares(lk, which)[pair][0] / _shares(lk, which)[pair][1])
    changed, n = _shares(best, which)[pair]
    carriers = [_pid(lk) for lk in PLANE_KEYS if _shares(lk, which)[pair][0] >= max(1000, 0.1 * _shares(lk, which)[pair][1])]
    print(f"[coverage] {which} without {pair}: {_pid(best)} differs in {changed} of {n} elements ({changed / n:.1%}); "
          f"{len(carriers)} cases carry it")
    assert changed >= 1000 and changed >= 0.1 * n, (which, pair, changed, n)
    assert carriers
