"""CPU: probability curves and flip points (VqaNet.explain_faithfulness_probs / explain_faithfulness_probs_pairs) -- the kept
form up to the hidden row, times W2 plus b2, then softmax, against a brute-force forward with the absent rows zeroed (float64);
the share of arg-max entries the GPU tests may leave out, on the float64 reference alone; the flip and area methods of
ProbabilityCurves; the two new entry points in the header, the ctypes prototypes and the built library with their host-side
argument validation."""
import itertools
import re

import pytest
import torch

from dl_vqa_amd import Faithfulness, ProbabilityCurves
from tests import attribution_ref as R
from tests import faithfulness_ref as FR
from tests import prob_curves_ref as PR
from tests.curves_util import _maps, _random_case
from tests.explain_util import columns as _columns

# The logit bound the CPU share test stands in for the one the GPU tests measure (4 x answer() on zeroed banks against
# float64, floor 1e-7; profiles/faithfulness_parity.txt has it AT the floor on all three fixtures): ten times the floor.
FIXTURE_LOGIT_BOUND = 1e-6


def _check_identity(tag, sd, do_option, vn, qf, img, cols, grid, maps):
    order = FR.rank_desc(maps)
    P = vn.shape[1]
    want = PR.brute_prob_curves(sd, do_option, vn, qf, img, cols, grid, order)
    got = PR.curve_stats(PR.closed_logit_curves(sd, do_option, vn, qf, img, order), cols)
    err = float((got["prob"] - want["prob"]).abs().max())
    err_top = float((got["top_prob"] - want["top_prob"]).abs().max())
    print(f"[identity-prob-curves] {tag}: kept form vs brute force, probability {err:.3e}, top probability {err_top:.3e}, "
          f"max probability {float(want['prob'].max()):.3e}")
    assert float(want["prob"].max()) > 0 and err < 1e-12 and err_top < 1e-12
    # the arg-max wherever the float64 margin is not itself a rounding error
    clear = want["margin"] > 1e-9
    assert torch.equal(got["top"][clear], want["top"][clear])
    # both ends: the full image and the empty image
    full = torch.softmax(R.forward64(sd, do_option, vn, qf, img, grid), -1).gather(1, torch.as_tensor(cols)[:, None])[:, 0]
    assert float((got["prob"][:, 0, 0] - full).abs().max()) < 1e-12 and float((got["prob"][:, 1, P] - full).abs().max()) < 1e-12
    assert torch.equal(got["prob"][:, 0, P], got["prob"][:, 1, 0])
    # the explained column of the logits is faithfulness_ref's logit curve
    d, i = FR.brute_curves(sd, do_option, vn, qf, img, cols, grid, order)
    picked = want["logits"].gather(-1, torch.as_tensor(cols).view(-1, 1, 1, 1).expand(-1, 2, P + 1, 1))[..., 0]
    assert torch.equal(picked[:, 0], d) and torch.equal(picked[:, 1], i)


@pytest.mark.parametrize("ties", [False, True], ids=["random", "ties"])
@pytest.mark.parametrize("do_option", ["+", "*", "|"])
def test_kept_hidden_rows_give_the_brute_force_probabilities_on_the_fixtures(do_option, ties):
    f = R.fixture_case(do_option)
    sd, A = f["golden"].sd, f["cfg"]["max_answers"]
    top = R.forward64(sd, do_option, f["vn"], f["qf"], f["img"], f["grid"]).argmax(1).tolist()
    for cols in (top, _columns(len(top), A)):
        _check_identity(R.FIXTURES[do_option], sd, do_option, f["vn"], f["qf"], f["img"], cols, f["grid"],
                        _maps(len(top), f["vn"].shape[1], 7, ties))


@pytest.mark.parametrize("ties", [False, True], ids=["random", "ties"])
@pytest.mark.parametrize("G", [1, 2])
@pytest.mark.parametrize("do_option", ["+", "*", "|"])
@pytest.mark.parametrize("grid", [(3, 4), (5, 7)])
def test_kept_hidden_rows_give_the_brute_force_probabilities_on_synthetic_grids(grid, do_option, G, ties):
    sd, vn, qf, img, answers = _random_case(do_option, G, grid, seed=100 * grid[0] + 10 * G + R.MODES[do_option])
    _check_identity(f"{grid} '{do_option}' G={G}", sd, do_option, vn, qf, img, answers, grid,
                    _maps(len(img), grid[0] * grid[1], 11 + G, ties))


@pytest.mark.parametrize("do_option", ["+", "*", "|"])
def test_the_float64_reference_leaves_out_at_most_5_per_cent_of_the_tops_for_any_ranking_of_a_fixture(do_option):
    """The GPU tests compare an fp32 arg-max with the float64 one only where the float64 margin exceeds four times the logit
    bound in force, and may leave out at most 5 % of a case's entries.  The fixtures have P = 4, so a ranking is one of 24
    permutations per question: whatever maps the GPU tests rank (explain_occlusion's, explain's, a random map with ties), the
    same permutation for every question is one of the 24 cases here and a mixed one is bounded by their worst rows."""
    f = R.fixture_case(do_option)
    B, P = len(f["img"]), f["vn"].shape[1]
    assert P == 4
    worst, worst_rows = 0.0, torch.zeros(B)
    for perm in itertools.permutations(range(P)):
        margin = PR.curve_stats(PR.fixture_brute_logit_curves(do_option, [list(perm)] * B), [0] * B)["margin"]
        mask, share = PR.comparable(margin, FIXTURE_LOGIT_BOUND)
        worst = max(worst, share)
        worst_rows = torch.maximum(worst_rows, 1.0 - mask.double().mean((1, 2)))
    mixed = float(worst_rows.mean())                                  # every question with the permutation that is worst for it
    print(f"[share-prob-curves] {R.FIXTURES[do_option]}: share of (b, k) entries with a float64 margin <= 4 x {FIXTURE_LOGIT_BOUND:g}: "
          f"worst single permutation {worst:.4f}, worst mix of permutations {mixed:.4f} (cap {PR.MAX_LEFT_OUT})")
    assert worst <= PR.MAX_LEFT_OUT and mixed <= PR.MAX_LEFT_OUT


# ----------------------------------------------------------------------------- the methods of the result
def _result(deletion_top, insertion_top, answers, deletion=None, insertion=None):
    dt, it = torch.tensor(deletion_top, dtype=torch.int32), torch.tensor(insertion_top, dtype=torch.int32)
    B, K = dt.shape
    z = torch.zeros(B, K)
    return ProbabilityCurves(z if deletion is None else deletion, z if insertion is None else insertion, dt, it, z, z,
                             torch.zeros(B, K - 1, dtype=torch.int64), torch.tensor(answers, dtype=torch.int64), torch.zeros(B, 9))


def test_flip_points_on_hand_made_tops():
    # P = 3: steps 0 .. 3, the sentinel is 4.  Rows: never flips, flips at 0, flips at P, flips at 1 and comes back
    res = _result(deletion_top=[[5, 5, 5, 5], [2, 5, 5, 5], [5, 5, 5, 1], [5, 0, 5, 5]],
                  insertion_top=[[1, 2, 3, 4], [5, 0, 0, 0], [0, 0, 0, 5], [0, 5, 0, 5]], answers=[5, 5, 5, 5])
    d, i = res.deletion_flip(), res.insertion_flip()
    assert d.dtype == i.dtype == torch.int64 and d.shape == i.shape == (4,)
    assert d.tolist() == [4, 0, 3, 1] and i.tolist() == [4, 0, 3, 1]
    # a column that no row ever reaches, an empty batch
    assert _result([[0, 1, 2, 3]], [[0, 1, 2, 3]], [7]).insertion_flip().tolist() == [4]
    assert _result([[0, 1, 2, 3]], [[0, 1, 2, 3]], [7]).deletion_flip().tolist() == [0]
    none = ProbabilityCurves(*(torch.zeros(0, 4) for _ in range(2)), *(torch.zeros(0, 4, dtype=torch.int32) for _ in range(2)),
                             *(torch.zeros(0, 4) for _ in range(2)), torch.zeros(0, 3, dtype=torch.int64),
                             torch.zeros(0, dtype=torch.int64), torch.zeros(0, 9))
    assert none.deletion_flip().shape == none.insertion_flip().shape == (0,) and none.deletion_flip().dtype == torch.int64
    assert none.deletion_auc().shape == (0,)


def test_auc_methods_are_faithfulness_own():
    g = torch.Generator().manual_seed(2)
    B, P = 4, 35
    d, i = torch.rand(B, P + 1, generator=g), torch.rand(B, P + 1, generator=g)
    res = _result([[0] * (P + 1)] * B, [[0] * (P + 1)] * B, [0] * B, d, i)
    ref = Faithfulness(d, i, res.order, res.answers, res.logits)
    assert torch.equal(res.deletion_auc(), ref.deletion_auc()) and torch.equal(res.insertion_auc(), ref.insertion_auc())
    assert res.deletion_auc().dtype == torch.float64
    assert float((res.insertion_auc() - torch.trapezoid(i.double(), dim=1) / P).abs().max()) < 1e-12
    assert ProbabilityCurves._fields == ("deletion", "insertion", "deletion_top", "insertion_top", "deletion_top_prob",
                                         "insertion_top_prob", "order", "answers", "logits")


# ----------------------------------------------------------------------------- the ABI
NEW = ("vqa_occl_curves_hidden", "vqa_softmax_pick")


def test_new_entry_points_are_declared_bound_and_exported_without_an_abi_bump():
    import os
    from dl_vqa_amd import _lib, build, ops
    build.build_library(verbose=False)
    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vqa_hip.h")).read()
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", header) and name in _lib.PROTOTYPES and hasattr(lib, name)
    assert _lib.header_abi_version() == 9 and lib.vqa_abi_version() == 9
    # declared behind the entry points they extend
    assert header.index("vqa_occl_curves_orders(") < header.index("vqa_occl_curves_hidden(")
    assert header.index("int vqa_softmax_topk(") < header.index("int vqa_softmax_pick(")
    assert callable(ops.occl_curves_hidden) and callable(ops.softmax_pick)


def test_occl_curves_hidden_argument_validation_without_gpu():
    import ctypes
    from dl_vqa_amd import _lib
    lib = _lib.load()
    err = lambda: lib.vqa_last_error()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p).value                       # a 16-byte aligned host address: never dereferenced
    assert p % 16 == 0
    f32 = lambda a: ctypes.cast(a, ctypes.POINTER(ctypes.c_float))

    def call(base=p, U=p, slot=p, probs=p, score=p, cnull=p, order=p, ws=p, ws_bytes=1 << 30, hidden=p, R=2, B=3, P=4, hid=20, G=2):
        return lib.vqa_occl_curves_hidden(f32(base), f32(U), slot, 0, f32(probs), f32(score), f32(cnull), order, f32(ws), ws_bytes,
                                          f32(hidden), R, B, P, hid, G, None)

    assert call(G=5) == 1 and b"vqa_occl_curves_hidden: glimpses=5" in err()
    assert call(hidden=None) == 1 and b"vqa_occl_curves_hidden: null pointer" in err()
    assert call(order=None) == 1 and b"null pointer" in err()
    assert call(hid=18) == 1 and b"multiple of 4" in err()
    assert call(P=0) == 1 and b"out of range" in err()
    assert call(R=0) == 1 and b"out of range" in err()
    assert call(hid=16384) == 1 and b"1*hid=16384 too large for LDS" in err()
    assert call(hidden=p + 4) == 1 and b"base, U, the workspace and the hidden rows must be 16-byte aligned" in err()
    assert call(ws_bytes=lib.vqa_occl_curves_workspace_bytes(3, 4, 2, 20) - 4) == 1 and b"workspace" in err()
    assert call(B=0, ws=None, ws_bytes=0) == 0                        # nothing to do: no launch, no workspace


def test_softmax_pick_argument_validation_without_gpu():
    import ctypes
    from dl_vqa_amd import _lib
    lib = _lib.load()
    err = lambda: lib.vqa_last_error()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p).value
    f32 = lambda a: ctypes.cast(a, ctypes.POINTER(ctypes.c_float))

    def call(logits=p, ld=8, rows=6, A=8, answers=p, rpq=2, top=p, top_prob=p, prob_at=p):
        return lib.vqa_softmax_pick(f32(logits), ld, rows, A, answers, rpq, top, f32(top_prob), f32(prob_at), None)

    assert call(ld=7) == 1 and b"vqa_softmax_pick" in err() and b"ld >= A" in err()
    assert call(A=0) == 1 and b"out of range" in err()
    assert call(rows=-1) == 1 and b"out of range" in err()
    assert call(rpq=0) == 1 and b"rows_per_question=0" in err()
    assert call(rpq=4) == 1 and b"divide rows=6" in err()
    for missing in ("logits", "answers", "top", "top_prob", "prob_at"):
        assert call(**{missing: None}) == 1 and b"null pointer" in err()
    assert call(rows=0, logits=None, answers=None, top=None, top_prob=None, prob_at=None) == 0
