"""CPU: occlusion maps from cached features (VqaNet.explain_occlusion / explain_occlusion_pairs) -- the closed form behind
vqa_occl_logit against a brute-force forward with the occluded features zeroed (float64), that the exact map is not a
restatement of the gradient x input map, the new entry point in the header, the ctypes prototypes and the built library with
its host-side argument validation, and the errors only these calls raise before any device work (the window; what explain /
explain_pairs raise for the same arguments).  The refusals every explain call shares: tests/test_explain_refusals_cpu.py."""
import re

import pytest
import torch

from dl_vqa_amd import ImageFeatures, Occlusion
from tests import attribution_ref as R
from tests import occlusion_ref as OR
from tests.curves_util import _random_case
from tests.explain_util import columns as _columns, host_caches as _host_caches, tiny as _tiny


# ----------------------------------------------------------------------------- the identity, in float64
@pytest.mark.parametrize("window", [1, 3])
@pytest.mark.parametrize("do_option", ["+", "*", "|"])
def test_closed_form_equals_brute_force_on_the_fixtures(do_option, window):
    f = R.fixture_case(do_option)
    sd, A = f["golden"].sd, f["cfg"]["max_answers"]
    assert f["vn"].shape[1] == 4                                  # a 2 x 2 grid: window 3 covers all of it from anywhere
    top = R.forward64(sd, do_option, f["vn"], f["qf"], f["img"], f["grid"]).argmax(1).tolist()
    for cols in (top, _columns(len(top), A)):
        want = OR.fixture_brute(do_option, cols, window)
        got, parts = OR.closed_form(sd, do_option, f["vn"], f["qf"], f["img"], cols, f["grid"], window)
        err = float((got - want).abs().max())
        print(f"[identity-occlusion] {R.FIXTURES[do_option]} window {window}: closed form vs brute force {err:.3e}, "
              f"max|map| {float(want.abs().max()):.3e}, max alpha {float(parts['alpha'].max()):.3f}")
        assert float(want.abs().max()) > 0 and err < 1e-12
        if window == 3:                                           # the whole grid: one value per question
            assert float((want - want[:, :1]).abs().max()) < 1e-12


@pytest.mark.parametrize("G", [1, 2])
@pytest.mark.parametrize("do_option", ["+", "*", "|"])
@pytest.mark.parametrize("grid", [(3, 4), (5, 7)])
def test_closed_form_equals_brute_force_on_synthetic_grids(grid, do_option, G):
    sd, vn, qf, img, answers = _random_case(do_option, G, grid, seed=100 * grid[0] + 10 * G + R.MODES[do_option])
    for window in (1, 3, 5):
        want = OR.brute(sd, do_option, vn, qf, img, answers, grid, window)
        got, parts = OR.closed_form(sd, do_option, vn, qf, img, answers, grid, window)
        err = float((got - want).abs().max())
        print(f"[identity-occlusion] {grid} '{do_option}' G={G} window {window}: closed form vs brute force {err:.3e}, "
              f"max|map| {float(want.abs().max()):.3e}, max alpha {float(parts['alpha'].max()):.3f}")
        assert float(want.abs().max()) > 0 and err < 1e-12
        assert float(parts["alpha"].min()) > 0
    # a window clipped at the border holds fewer positions: the corner of a 3-wide window has 4, the centre 9
    counts = OR.windows(*grid, 3).sum(-1)
    assert counts[0] == 4 and counts.max() == 9


@pytest.mark.parametrize("do_option", ["+", "*", "|"])
def test_the_occlusion_map_is_not_the_gradient_x_input_map(do_option):
    """The exact map and its first-order estimate differ by more than 5 % of the exact map's maximum on every fixture."""
    f = R.fixture_case(do_option)
    sd = f["golden"].sd
    top = R.forward64(sd, do_option, f["vn"], f["qf"], f["img"], f["grid"]).argmax(1).tolist()
    exact = OR.fixture_brute(do_option, top, 1)
    first_order = R.autograd_reference(sd, do_option, f["vn"], f["qf"], f["img"], top, f["grid"])
    gap = float((exact - first_order).abs().max()) / float(exact.abs().max())
    print(f"[identity-occlusion] {R.FIXTURES[do_option]}: |occlusion - gradient x input| = {gap:.3f} of max|occlusion| = "
          f"{float(exact.abs().max()):.3e}")
    assert gap > 0.05


# ----------------------------------------------------------------------------- the ABI
def test_new_entry_point_in_header_prototypes_and_library():
    from dl_vqa_amd import _lib, build
    build.build_library(verbose=False)
    with open(_lib.HEADER_PATH) as f:
        header = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    assert re.search(r"\bvqa_occl_logit\s*\(", header) and "vqa_occl_logit" in _lib.PROTOTYPES
    lib = _lib.load()
    assert lib.vqa_abi_version() == _lib.header_abi_version() == 9          # appended, not bumped
    assert hasattr(lib, "vqa_occl_logit")
    from dl_vqa_amd import ops
    assert callable(ops.occl_logit)


def test_occl_logit_argument_validation_without_gpu():
    """base, Z, U, slot, slot0, probs, score, cnull, W2, w2_ld, b2, answers, logits, logits_ld, maps, R, B, gh, gw, hid, G, A,
    window, stream (pointers are made-up aligned integers: every check runs on the host before any HIP call)."""
    from dl_vqa_amd import _lib
    lib = _lib.load()
    err = lib.vqa_last_error
    f = lib.vqa_occl_logit
    ok = dict(base=16, Z=16, U=16, slot=16, slot0=0, probs=16, score=16, cnull=16, W2=16, w2_ld=20, b2=16, answers=16, logits=16,
              logits_ld=12, maps=16, R=2, B=3, gh=2, gw=2, hid=20, G=2, A=12, window=1, stream=None)

    def call(**kw):
        return f(*{**ok, **kw}.values())

    assert call(B=0) == 0                                             # nothing to do, nothing launched
    assert call(hid=18, B=0) == 1 and b"multiple of 4" in err() and b"hid=18" in err()
    assert call(w2_ld=16, B=0) == 1 and b"w2_ld" in err()             # w2_ld < hid
    assert call(G=5, B=0) == 1 and b"glimpses" in err()
    for window in (0, 2, 9, -1):
        assert call(window=window, B=0) == 1 and b"window" in err()
    for name in ("base", "Z", "U", "slot", "probs", "score", "cnull", "W2", "b2", "answers", "logits", "maps"):
        assert call(**{name: None}, B=0) == 1 and b"null pointer" in err(), name
    for name in ("base", "Z", "U", "W2"):
        assert call(**{name: 20}, B=0) == 1 and b"aligned" in err(), name
    assert call(R=0, B=0) == 1 and b"out of range" in err()
    assert call(logits_ld=11, B=0) == 1 and b"out of range" in err()  # logits_ld < A
    assert call(hid=4096, w2_ld=4096, G=4, B=0) == 1 and b"LDS" in err()


# ----------------------------------------------------------------------------- errors before any device work
# (what the six explain calls refuse alike: tests/test_explain_refusals_cpu.py)
def test_window_answers_and_features_are_judged_before_any_device_work():
    assert Occlusion._fields == ("maps", "answers", "logits")
    g, m = _tiny()
    m.eval()
    feats, qfeats = _host_caches(m, N=3, M=2)
    q, ql = g.t["q"][:3], g.t["q_len"][:3]
    single = lambda **kw: m.explain_occlusion(feats, q, ql, [0, 1, 2], **kw)
    pairs = lambda **kw: m.explain_occlusion_pairs(feats, qfeats, [0, 1, 2], [0, 1, 1], **kw)
    for call in (single, pairs):
        for window in (0, 2, 4, 9, -1, True, 3.0, "3", None):
            with pytest.raises(ValueError, match="window must be an odd int in 1..7"):
                call(window=window)
    # an index out of range, features without v' and foreign features: whatever explain / explain_pairs raise for the same
    # arguments on this host (the device checks of the GPU tests judge them where a device is present), word for word
    bank = ImageFeatures(torch.zeros(3, 4, m._engine.C), None, (2, 2), m)
    _, other = _tiny()
    other.eval()
    theirs, their_q = _host_caches(other)

    def raised(call):
        with pytest.raises(Exception) as e:
            call()
        return type(e.value), str(e.value).replace("explain_occlusion", "explain")

    for images in (feats, bank, theirs):
        for index in ([0, 1, 2], [0, 1, feats.N]):
            assert raised(lambda: m.explain_occlusion(images, q, ql, index)) == raised(lambda: m.explain(images, q, ql, index))
            for questions in (qfeats, their_q):
                assert raised(lambda: m.explain_occlusion_pairs(images, questions, index, [0, 1, 1])) == \
                    raised(lambda: m.explain_pairs(images, questions, index, [0, 1, 1]))
    with pytest.raises(IndexError):
        m.explain_occlusion_pairs(feats, qfeats, [0, 1, feats.N], [0, 1, 1])
    assert m._last_ctx is None and all(p.grad is None for p in m.parameters())
