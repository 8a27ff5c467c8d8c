"""CPU: sampled Shapley maps (VqaNet.explain_shapley / explain_shapley_pairs) in float64 -- the kept-form route against a forward
per subset, completeness, the half of all orders plus their reverses against all permutations, the reversal identity of the
curves, shapley_orders, the seed of the GPU sampling test, the new entry points in the header, the prototypes and the library
with their host-side argument validation, and how far explain's and explain_occlusion's maps are from the Shapley value."""
import re

import pytest
import torch

from dl_vqa_amd import IntegratedGradients, Shapley, shapley_orders
from tests import attribution_ref as R
from tests import occlusion_ref as OR
from tests import shapley_ref as SR
from tests.explain_util import columns as _columns


def _fixture(do_option):
    f = R.fixture_case(do_option)
    sd, A = f["golden"].sd, f["cfg"]["max_answers"]
    top = R.forward64(sd, do_option, f["vn"], f["qf"], f["img"], f["grid"]).argmax(1).tolist()
    return f, sd, (top, _columns(len(top), A))


# ----------------------------------------------------------------------------- the identities, in float64
@pytest.mark.parametrize("do_option", ["+", "*", "|"])
def test_closed_form_equals_brute_force_is_complete_and_half_the_orders_with_reverses_are_exact(do_option):
    f, sd, column_sets = _fixture(do_option)
    P = f["vn"].shape[1]
    assert P == 4 and f["grid"] == (2, 2)
    half = SR.half_orders(P)
    assert half.shape == (12, 4)
    for cols in column_sets:
        args = (sd, do_option, f["vn"], f["qf"], f["img"], cols, f["grid"])
        closed = SR.fixture_exact(do_option, cols)
        brute = SR.exact_from_state_dict(*args, brute=True)           # a forward per kept set of every permutation
        err = float((closed - brute).abs().max())
        full = R.forward64(*args[:5], f["grid"]).gather(1, torch.as_tensor(cols)[:, None])[:, 0]
        deletion, insertion = SR.curves_from_state_dict(*args, half)
        empty = insertion[:, 0, 0]
        assert float((insertion[:, :, 0] - empty[:, None]).abs().max()) == 0.0
        gap = float((closed.sum(1) - (full - empty)).abs().max())
        maps, stderr = SR.sampled(SR.estimates(deletion, insertion, half))
        pairs = float((maps - closed).abs().max())
        print(f"[shapley] {R.FIXTURES[do_option]}: closed form vs brute force {err:.3e}, completeness {gap:.3e}, 12 orders + "
              f"reverses vs 24 permutations {pairs:.3e}, max|phi| {float(closed.abs().max()):.3e}")
        assert float(closed.abs().max()) > 0 and err < 1e-12 and gap < 1e-12 and pairs < 1e-12
        assert float((maps.sum(1) - (full - empty)).abs().max()) < 1e-12 and bool((stderr >= 0).all())


def test_the_reversed_orders_insertion_curve_is_the_deletion_curve_read_backwards():
    c = SR.case((3, 2, 2, 3, 2, 20, 5))
    orders = c["orders"]
    deletion, insertion = SR.curves_for_orders(*SR.operands(c), orders)
    _, reversed_insertion = SR.curves_for_orders(*SR.operands(c), orders.flip(1))
    assert float((reversed_insertion - deletion.flip(2)).abs().max()) < 1e-12
    # hence each estimate is the mean of the marginals under the order and under its reverse
    e = SR.estimates(deletion, insertion, orders)
    forward = insertion[..., 1:] - insertion[..., :-1]
    backward = reversed_insertion[..., 1:] - reversed_insertion[..., :-1]
    both = torch.zeros_like(e).scatter_(2, orders[None].expand_as(e), forward) \
        + torch.zeros_like(e).scatter_(2, orders.flip(1)[None].expand_as(e), backward)
    assert float((e - 0.5 * both).abs().max()) < 1e-12


@pytest.mark.parametrize("P", [4, 5])
def test_half_orders_with_reverses_are_exact_on_synthetic_operands(P):
    half = SR.half_orders(P)
    assert half.shape[0] == {4: 12, 5: 60}[P]
    c = SR.case((3, 2, 1, P, 2, 20, half.shape[0]))
    e, _, _ = SR.pair_estimates(*SR.operands(c), half)
    assert float((SR.sampled(e)[0] - SR.exact(*SR.operands(c))).abs().max()) < 1e-12


def test_sampled_is_the_mean_and_the_standard_error_and_nan_for_one_order():
    e = torch.randn(3, 7, 5, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    maps, stderr = SR.sampled(e)
    assert float((maps - e.mean(1)).abs().max()) < 1e-15
    assert float((stderr - e.std(1, unbiased=True) / 7 ** 0.5).abs().max()) < 1e-15
    one = SR.sampled(e[:, :1])
    assert torch.equal(one[0], e[:, 0]) and bool(torch.isnan(one[1]).all())


# ----------------------------------------------------------------------------- the table of orders
def test_shapley_orders_is_deterministic_and_every_row_is_a_permutation():
    rng = torch.get_rng_state()
    a = shapley_orders(16, 35, 3)
    assert torch.equal(torch.get_rng_state(), rng)                    # a generator of its own
    assert a.dtype == torch.int64 and a.shape == (8, 35) and not a.is_cuda
    assert torch.equal(a.sort(1).values, torch.arange(35).expand(8, 35))
    assert torch.equal(a, shapley_orders(16, 35, 3)) and not torch.equal(a, shapley_orders(16, 35, 4))
    assert torch.equal(shapley_orders(16, 35), shapley_orders(16, 35, 0))
    assert torch.equal(shapley_orders(4, 35, 3), a[:2])               # one stream, drawn in ascending m
    gen = torch.Generator().manual_seed(3)
    assert torch.equal(a[0], torch.randperm(35, generator=gen)) and torch.equal(a[1], torch.randperm(35, generator=gen))
    assert shapley_orders(2, 1).tolist() == [[0]]


def test_the_seed_of_the_gpu_sampling_test_keeps_the_float64_reference_within_three_standard_errors():
    """The GPU test asks |maps - exact| <= 4 stderr of 32 drawn orders at P = 6; the seed is one for which the float64 estimate
    alone stays at or below 3."""
    B, Rr, gh, gw, G, hid, M = SR.SAMPLING_SHAPE
    P = gh * gw
    assert P == 6 and M == 32
    c = SR.case(SR.SAMPLING_SHAPE)
    exact = SR.exact(*SR.operands(c))
    orders = shapley_orders(2 * M, P, SR.SAMPLING_SEED)
    maps, stderr = SR.sampled(SR.pair_estimates(*SR.operands(c), orders)[0])
    ratio = float(((maps - exact).abs() / stderr).max())
    print(f"[shapley] P = 6, 32 orders of seed {SR.SAMPLING_SEED}: max |maps - exact| / stderr = {ratio:.2f} (float64), "
          f"max stderr {float(stderr.max()):.3e}, max|phi| {float(exact.abs().max()):.3e}")
    assert ratio <= 3.0 and float(stderr.min()) > 0


# ----------------------------------------------------------------------------- the result type
def test_shapley_fields_and_the_completeness_gap():
    assert Shapley._fields == ("maps", "stderr", "answers", "logits", "baseline_logits")
    g = torch.Generator().manual_seed(4)
    maps, logits, base = torch.randn(3, 2, 2, generator=g), torch.randn(3, 5, generator=g), torch.randn(3, generator=g)
    cols = torch.tensor([4, 0, 2])
    res = Shapley(maps, torch.zeros(3, 2, 2), cols, logits, base)
    want = maps.double().sum((1, 2)) - (logits.double()[torch.arange(3), cols] - base.double())
    assert res.completeness_gap().dtype == torch.float64 and float((res.completeness_gap() - want).abs().max()) < 1e-15
    assert torch.equal(res.completeness_gap(), IntegratedGradients(maps, cols, logits, base).completeness_gap())


# ----------------------------------------------------------------------------- the ABI
NEW = ("vqa_occl_curves_orders_workspace_bytes", "vqa_occl_curves_orders", "vqa_shapley_accumulate")


def test_new_entry_points_in_header_prototypes_and_library():
    from dl_vqa_amd import _lib, build, ops
    build.build_library(verbose=False)
    with open(_lib.HEADER_PATH) as f:
        header = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    lib = _lib.load()
    assert lib.vqa_abi_version() == _lib.header_abi_version() == 9          # appended, not bumped
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", header) and name in _lib.PROTOTYPES and hasattr(lib, name), name
    assert callable(ops.occl_curves_orders) and callable(ops.occl_curves_orders_workspace) and callable(ops.shapley_accumulate)
    one = lib.vqa_occl_curves_workspace_bytes(3, 35, 2, 1024)
    assert lib.vqa_occl_curves_orders_workspace_bytes(3, 1, 35, 2, 1024) == one
    assert lib.vqa_occl_curves_orders_workspace_bytes(3, 8, 35, 2, 1024) == 8 * one
    assert lib.vqa_occl_curves_orders_workspace_bytes(3, 0, 35, 2, 1024) == 0


def test_occl_curves_orders_argument_validation_without_gpu():
    """base, U, slot, slot0, probs, score, cnull, W2, w2_ld, b2, answers, orders, workspace, workspace_bytes, deletion,
    insertion, R, B, M, P, hid, G, A, stream (pointers are made-up aligned integers: every check runs on the host before any HIP
    call)."""
    from dl_vqa_amd import _lib
    lib = _lib.load()
    err = lib.vqa_last_error
    f = lib.vqa_occl_curves_orders
    ok = dict(base=16, U=16, slot=16, slot0=0, probs=16, score=16, cnull=16, W2=16, w2_ld=20, b2=16, answers=16, orders=16,
              workspace=16, workspace_bytes=1 << 20, deletion=16, insertion=16, R=2, B=0, M=3, P=4, hid=20, G=2, A=12, stream=None)

    def call(**kw):
        return f(*{**ok, **kw}.values())

    assert call() == 0                                                # B == 0: nothing to do, nothing launched
    assert call(workspace=None, workspace_bytes=0) == 0               # ... and no workspace needed
    assert call(M=0) == 1 and b"M=0" in err()
    assert call(M=-1) == 1 and b"M=-1" in err()
    assert call(B=1 << 20, M=1 << 11) == 1 and b"out of range" in err()     # B * M reaches 2^31
    assert call(hid=18) == 1 and b"multiple of 4" in err()
    assert call(w2_ld=16) == 1 and b"w2_ld" in err()
    assert call(G=9) == 1 and b"glimpses" in err()
    for name in ("base", "U", "slot", "probs", "score", "cnull", "W2", "b2", "answers", "orders", "deletion", "insertion"):
        assert call(**{name: None}) == 1 and b"null pointer" in err(), name
    assert call(R=0) == 1 and b"out of range" in err()
    assert call(P=0) == 1 and b"out of range" in err()
    assert call(hid=8192, w2_ld=8192) == 1 and b"LDS" in err()
    assert call(B=3, workspace=None) == 1 and b"workspace" in err()
    need = lib.vqa_occl_curves_orders_workspace_bytes(3, 3, 4, 2, 20)
    assert call(B=3, workspace_bytes=need - 4) == 1 and b"workspace" in err() and str(need).encode() in err()
    for name in ("base", "U", "W2", "workspace"):
        assert call(B=3, **{name: 20}) == 1 and b"aligned" in err(), name
    # the grid of the walk: B * M tasks x groups of chunks
    assert call(B=1 << 19, M=1 << 11, P=1 << 10, workspace_bytes=1 << 62) == 1 and b"exceed the grid" in err()


def test_shapley_accumulate_argument_validation_without_gpu():
    """deletion, insertion, rank, slot, slot0, answers, mean, m2, maps, err, empty, R, B, P, Mg, m0, total, A, stream."""
    from dl_vqa_amd import _lib
    lib = _lib.load()
    err = lib.vqa_last_error
    f = lib.vqa_shapley_accumulate
    ok = dict(deletion=16, insertion=16, rank=16, slot=16, slot0=0, answers=16, mean=16, m2=16, maps=16, err=16, empty=16, R=2,
              B=0, P=4, Mg=3, m0=0, total=3, A=12, stream=None)

    def call(**kw):
        return f(*{**ok, **kw}.values())

    assert call() == 0                                                # B == 0: nothing launched
    assert call(total=0, maps=None, err=None, empty=None) == 0        # a group that is not the last writes the state alone
    for name in ("deletion", "insertion", "rank", "slot", "answers", "mean", "m2", "maps", "err"):
        assert call(**{name: None}) == 1 and b"null pointer" in err(), name
    assert call(Mg=0) == 1 and b"Mg=0" in err()
    assert call(m0=-1) == 1 and b"m0=-1" in err()
    assert call(total=2) == 1 and b"total=2" in err()                 # neither 0 nor m0 + Mg
    assert call(m0=2, total=5) == 0
    assert call(P=0) == 1 and b"out of range" in err()
    assert call(R=0) == 1 and b"out of range" in err()
    assert call(A=0) == 1 and b"out of range" in err()
    assert call(B=-1) == 1 and b"out of range" in err()


# ----------------------------------------------------------------------------- what the other maps miss (recorded, not asserted)
@pytest.mark.parametrize("do_option", ["+", "*", "|"])
def test_print_how_far_explain_and_explain_occlusion_are_from_the_shapley_value(do_option):
    f, sd, column_sets = _fixture(do_option)
    cols = column_sets[0]
    phi = SR.fixture_exact(do_option, cols)
    grad = R.fixture_reference(do_option, cols)[0]
    occl = OR.fixture_brute(do_option, cols, 1)
    scale = float(phi.abs().max())
    for name, other in (("explain", grad), ("explain_occlusion", occl)):
        diff = float((other.reshape(phi.shape) - phi).abs().max())
        print(f"[shapley] {R.FIXTURES[do_option]}: {name} vs exact Shapley, max|diff| = {diff:.3e} = {diff / scale:.2f} x max|phi| "
              f"({scale:.3e}); sums {float(other.sum(1).abs().max()):.3e} vs {float(phi.sum(1).abs().max()):.3e}")
    assert scale > 0
