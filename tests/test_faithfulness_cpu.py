"""CPU: deletion and insertion curves of an attribution map (VqaNet.explain_faithfulness / explain_faithfulness_pairs) -- the
kept form behind vqa_occl_curves against a brute-force forward with the absent rows zeroed (float64), the ranking's total order,
the new entry points in the header, the ctypes prototypes and the built library with their host-side argument validation, the
areas under the curves, and the errors these calls raise before any device work (the maps argument; the family's refusals)."""
import re

import pytest
import torch

from dl_vqa_amd import Faithfulness, ImageFeatures
from tests import attribution_ref as R
from tests import faithfulness_ref as FR
from tests.curves_util import _maps, _random_case
from tests.explain_util import columns as _columns, host_caches as _host_caches, tiny as _tiny


def _check_identity(tag, sd, do_option, vn, qf, img, cols, grid, maps):
    order = FR.rank_desc(maps)
    P = vn.shape[1]
    assert torch.equal(order.sort(1).values, torch.arange(P).expand_as(order))
    want_d, want_i = FR.brute_curves(sd, do_option, vn, qf, img, cols, grid, order)
    got_d, got_i, parts = FR.closed_curves(sd, do_option, vn, qf, img, cols, grid, order)
    err = max(float((got_d - want_d).abs().max()), float((got_i - want_i).abs().max()))
    print(f"[identity-faithfulness] {tag}: kept form vs brute force {err:.3e}, max|curve| {float(want_d.abs().max()):.3e}, "
          f"max alpha {float(max(parts['alpha_del'].max(), parts['alpha_ins'].max())):.3f}")
    assert float(want_d.abs().max()) > 0 and err < 1e-12
    full = R.forward64(sd, do_option, vn, qf, img, grid).gather(1, torch.as_tensor(cols)[:, None])[:, 0]
    assert float((got_d[:, 0] - full).abs().max()) < 1e-12 and float((got_i[:, P] - full).abs().max()) < 1e-12
    assert torch.equal(got_d[:, P], got_i[:, 0])
    assert float((want_d[:, P] - want_i[:, 0]).abs().max()) == 0.0


# ----------------------------------------------------------------------------- the identity, in float64
@pytest.mark.parametrize("ties", [False, True], ids=["random", "ties"])
@pytest.mark.parametrize("do_option", ["+", "*", "|"])
def test_kept_form_equals_brute_force_on_the_fixtures(do_option, ties):
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
def test_kept_form_equals_brute_force_on_synthetic_grids(grid, do_option, G, ties):
    sd, vn, qf, img, answers = _random_case(do_option, G, grid, seed=100 * grid[0] + 10 * G + R.MODES[do_option])
    _check_identity(f"{grid} '{do_option}' G={G}", sd, do_option, vn, qf, img, answers, grid,
                    _maps(len(img), grid[0] * grid[1], 11 + G, ties))


def test_sequential_restatement_equals_the_kept_form_in_float64():
    """The order of sums the kernel follows, restated on the host, is the kept form: whatever the chunk length."""
    sd, vn, qf, img, answers = _random_case("+", 2, (5, 7), seed=3)
    order = FR.rank_desc(_maps(len(img), 35, 5, False))
    _, _, parts = FR.closed_curves(sd, "+", vn, qf, img, answers, (5, 7), order)
    G, C = 2, vn.shape[2]
    w1 = sd["classifier.lin1.weight"]
    hid = w1.shape[0]
    vn_, vp, qp, wx, bx, _d, _, mode = R.model_inputs(sd, "+", vn, qf, img, answers)
    score, _ = R.scores(vp, qp, wx, bx, img, mode)
    probs = torch.softmax(score, -1)
    cnull = torch.relu(qp) @ wx.t() + bx
    U = torch.einsum("hgc,npc->npgh", w1[:, :G * C].reshape(hid, G, C), vn_)
    base = sd["classifier.lin1.bias"] + qf @ w1[:, G * C:].t()
    for L in (1, 4, 16, 35, 64):
        d, i = FR.sequential_curves(base, U, img, probs, score, cnull, sd["classifier.lin2.weight"], sd["classifier.lin2.bias"],
                                    answers, order, L, torch.float64)
        assert float((d - parts["deletion"]).abs().max()) < 1e-12 and float((i - parts["insertion"]).abs().max()) < 1e-12


# ----------------------------------------------------------------------------- the ranking
def test_rank_desc_is_one_total_order():
    nan, inf = float("nan"), float("inf")
    rows = torch.tensor([[1.0, 3.0, 2.0, 3.0, 1.0, 0.5],              # ties by the smaller position
                         [0.0, -0.0, 1.0, -0.0, 0.0, -1.0],           # signed zeros are equal
                         [nan, -inf, 2.0, nan, inf, -0.0],            # every NaN behind -inf, by position
                         [4.0, 4.0, 4.0, 4.0, 4.0, 4.0]])             # a constant row: the identity
    assert FR.rank_desc(rows).tolist() == [[1, 3, 2, 0, 4, 5], [2, 0, 1, 3, 4, 5], [4, 2, 5, 1, 0, 3], [0, 1, 2, 3, 4, 5]]
    assert FR.rank_desc(torch.full((2, 5), nan)).tolist() == [[0, 1, 2, 3, 4]] * 2
    # torch.topk's values on a row without ties or NaN
    v = torch.randn(3, 40, generator=torch.Generator().manual_seed(1))
    assert torch.equal(FR.rank_desc(v), torch.sort(v, 1, descending=True).indices)


def test_kept_sets_count_steps_and_skip_entries_out_of_range():
    deletion, insertion = FR.kept_sets(torch.tensor([[2, 7, 0, -1]]), 4)
    assert insertion[0].tolist() == [[0, 0, 0, 0], [0, 0, 1, 0], [0, 0, 1, 0], [1, 0, 1, 0], [1, 0, 1, 0]]
    assert deletion[0].tolist() == [[1, 0, 1, 0], [1, 0, 0, 0], [1, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]]


# ----------------------------------------------------------------------------- the areas
def test_auc_methods_are_the_float64_trapezoid_mean():
    g = torch.Generator().manual_seed(2)
    B, P = 4, 35
    d, i = torch.randn(B, P + 1, generator=g), torch.randn(B, P + 1, generator=g)
    res = Faithfulness(d, i, torch.zeros(B, P, dtype=torch.int64), torch.zeros(B, dtype=torch.int64), torch.zeros(B, 3))
    for got, curve in ((res.deletion_auc(), d), (res.insertion_auc(), i)):
        want = torch.tensor([sum((float(c[k]) + float(c[k + 1])) / (2 * P) for k in range(P)) for c in curve], dtype=torch.float64)
        assert got.dtype == torch.float64 and got.shape == (B,) and float((got - want).abs().max()) < 1e-12
        assert float((got - torch.trapezoid(curve.double(), dim=1) / P).abs().max()) < 1e-12


# ----------------------------------------------------------------------------- the ABI
NEW = ("vqa_rank_desc", "vqa_occl_curves_chunk", "vqa_occl_curves_workspace_bytes", "vqa_occl_curves")


def test_new_entry_points_in_header_prototypes_and_library():
    from dl_vqa_amd import _lib, build, ops
    build.build_library(verbose=False)
    with open(_lib.HEADER_PATH) as f:
        header = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    lib = _lib.load()
    assert lib.vqa_abi_version() == _lib.header_abi_version() == 9          # appended, not bumped
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", header) and name in _lib.PROTOTYPES and hasattr(lib, name), name
    assert callable(ops.rank_desc) and callable(ops.occl_curves)
    L = lib.vqa_occl_curves_chunk()
    assert 1 <= L <= 63 and ops.occl_curves_chunk() == L
    # two arrays of chunk sums and two of chunk masses
    assert lib.vqa_occl_curves_workspace_bytes(3, 35, 2, 1024) == 2 * 3 * -(-35 // L) * 2 * 1025 * 4
    assert lib.vqa_occl_curves_workspace_bytes(0, 35, 2, 1024) == 0


def test_rank_desc_argument_validation_without_gpu():
    from dl_vqa_amd import _lib
    lib = _lib.load()
    err = lib.vqa_last_error
    f = lib.vqa_rank_desc                                             # maps, order, B, P, stream
    assert f(16, 16, 0, 4, None) == 0                                 # nothing to do, nothing launched
    assert f(None, 16, 0, 4, None) == 1 and b"null pointer" in err()
    assert f(16, None, 0, 4, None) == 1 and b"null pointer" in err()
    assert f(16, 16, 0, 8193, None) == 1 and b"out of range" in err() and b"P=8193" in err()
    assert f(16, 16, 0, 0, None) == 1 and b"out of range" in err()
    assert f(16, 16, -1, 4, None) == 1 and b"out of range" in err()
    assert f(16, 16, 0, 8192, None) == 0


def test_occl_curves_argument_validation_without_gpu():
    """base, U, slot, slot0, probs, score, cnull, W2, w2_ld, b2, answers, order, workspace, workspace_bytes, deletion,
    insertion, R, B, P, hid, G, A, stream (pointers are made-up aligned integers: every check runs on the host before any HIP
    call)."""
    from dl_vqa_amd import _lib
    lib = _lib.load()
    err = lib.vqa_last_error
    f = lib.vqa_occl_curves
    ok = dict(base=16, U=16, slot=16, slot0=0, probs=16, score=16, cnull=16, W2=16, w2_ld=20, b2=16, answers=16, order=16,
              workspace=16, workspace_bytes=1 << 20, deletion=16, insertion=16, R=2, B=0, P=4, hid=20, G=2, A=12, stream=None)

    def call(**kw):
        return f(*{**ok, **kw}.values())

    assert call() == 0                                                # B == 0: nothing to do, nothing launched
    assert call(workspace=None, workspace_bytes=0) == 0               # ... and no workspace needed
    assert call(hid=6) == 1 and b"multiple of 4" in err() and b"hid=6" in err()
    assert call(hid=18) == 1 and b"multiple of 4" in err()
    assert call(w2_ld=16) == 1 and b"w2_ld" in err()                  # w2_ld < hid
    assert call(G=9) == 1 and b"glimpses" in err()
    assert call(G=0) == 1 and b"glimpses" in err()
    for name in ("base", "U", "slot", "probs", "score", "cnull", "W2", "b2", "answers", "order", "deletion", "insertion"):
        assert call(**{name: None}) == 1 and b"null pointer" in err(), name
    assert call(R=0) == 1 and b"out of range" in err()
    assert call(P=0) == 1 and b"out of range" in err()
    assert call(hid=8192, w2_ld=8192) == 1 and b"LDS" in err()
    # with questions to answer: the workspace and the alignments are judged, still before any HIP call
    assert call(B=3, workspace=None) == 1 and b"workspace" in err()
    assert call(B=3, workspace_bytes=lib.vqa_occl_curves_workspace_bytes(3, 4, 2, 20) - 4) == 1 and b"workspace" in err()
    for name in ("base", "U", "W2", "workspace"):
        assert call(B=3, **{name: 20}) == 1 and b"aligned" in err(), name


# ----------------------------------------------------------------------------- errors before any device work
def test_maps_answers_and_features_are_judged_before_any_device_work():
    assert Faithfulness._fields == ("deletion", "insertion", "order", "answers", "logits")
    g, m = _tiny()
    m.eval()
    A = m._engine.A
    feats, qfeats = _host_caches(m, N=3, M=2)
    q, ql = g.t["q"][:3], g.t["q_len"][:3]
    good = torch.zeros(3, 2, 2)
    single = lambda maps=good, index=(0, 1, 2), **kw: m.explain_faithfulness(feats, q, ql, list(index), maps, **kw)
    pairs = lambda maps=good, index=(0, 1, 2), **kw: m.explain_faithfulness_pairs(feats, qfeats, list(index), [0, 1, 1], maps, **kw)
    for name, call in (("explain_faithfulness", single), ("explain_faithfulness_pairs", pairs)):
        for bad in (torch.zeros(3, 4, dtype=torch.int64), torch.zeros(3, 2, 2, dtype=torch.bool), [[1, 2, 3, 4]] * 3):
            with pytest.raises(TypeError, match=f"VqaNet.{name}: maps must be a floating tensor"):
                call(bad)
        for bad in (torch.zeros(3, 5), torch.zeros(2, 2, 2), torch.zeros(12), torch.zeros(4, 3), torch.zeros(3, 4, 1),
                    torch.zeros(3, 1, 4), torch.zeros(3, 2, 2, dtype=torch.float64)[:2]):
            with pytest.raises(ValueError, match=f"VqaNet.{name}: maps of shape"):
                call(bad)
        # the maps are judged before the answers, the answers before the index
        with pytest.raises(ValueError, match="maps of shape"):
            call(torch.zeros(3, 5), answers=[0, 1])
        with pytest.raises(ValueError, match="2 answers for 3"):
            call(answers=[0, 1])
        with pytest.raises(IndexError, match=rf"answers entry {A} out of range \[0, {A}\)"):
            call(answers=[0, A, 1])
        with pytest.raises(TypeError, match="integer"):
            call(answers=[0.0, 1.0, 2.0])
        if call is pairs:                                             # answer_pairs judges the index on the host
            with pytest.raises(IndexError):
                call(index=(0, 1, feats.N))
        # everything the host can judge is in order, in every accepted form of the maps: the device check speaks
        for fine in (good, torch.zeros(3, 4), torch.zeros(3, 4, dtype=torch.float64), torch.zeros(3, 2, 2, dtype=torch.float16)):
            with pytest.raises(RuntimeError, match="cuda"):
                call(fine, answers=[0, A - 1, 1], _u_bytes=64)
    # a grid above the rank kernel's cap
    big = ImageFeatures(torch.zeros(1, 8281, m._engine.C), torch.zeros(8281, m._engine.mid), (91, 91), m)
    with pytest.raises(ValueError, match="8281 grid positions, the ranking takes at most 8192"):
        m.explain_faithfulness(big, q[:1], ql[:1], [0], torch.zeros(1, 91, 91))
    with pytest.raises(ValueError, match="8281 grid positions"):
        m.explain_faithfulness_pairs(big, qfeats, [0], [0], torch.zeros(1, 8281))
    # features that are no ImageFeatures, a bank without v' and foreign features: explain's words
    with pytest.raises(TypeError, match="encode_images"):
        m.explain_faithfulness(torch.zeros(3), q, ql, [0, 1, 2], good)
    with pytest.raises(TypeError, match="encode_questions"):
        m.explain_faithfulness_pairs(feats, feats, [0, 1, 2], [0, 1, 1], good)
    bank = _host_caches(m, vprime=False)[0]
    _, other = _tiny()
    other.eval()
    theirs, their_q = _host_caches(other)

    def raised(call, name):
        with pytest.raises(Exception) as e:
            call()
        return type(e.value), str(e.value).replace(name, "explain")

    for images in (bank, theirs):
        assert raised(lambda: m.explain_faithfulness(images, q, ql, [0, 1, 2], good), "explain_faithfulness") == \
            raised(lambda: m.explain(images, q, ql, [0, 1, 2]), "explain")
        for questions in (qfeats, their_q):
            assert raised(lambda: m.explain_faithfulness_pairs(images, questions, [0, 1, 2], [0, 1, 1], good),
                          "explain_faithfulness_pairs") == \
                raised(lambda: m.explain_pairs(images, questions, [0, 1, 2], [0, 1, 1]), "explain_pairs")
    assert m._last_ctx is None and all(p.grad is None for p in m.parameters())
