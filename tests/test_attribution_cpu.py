"""CPU: gradient x input maps from cached features (VqaNet.explain / explain_pairs) -- the identity behind the closed form
(float64, against autograd through the oracle's differentiable pieces), the condition under which the GPU tests on the golden
fixtures are meaningful (no ReLU pre-activation within rounding of zero), the new entry points in the header, the ctypes
prototypes and the built library with their host-side argument validation.  (The errors the public calls raise before any
device work: tests/test_explain_refusals_cpu.py.)"""
import re

import pytest
import torch

from dl_vqa_amd import Attribution
from tests import attribution_ref as R
from tests.explain_util import _random_case

NEW_ENTRY_POINTS = ("vqa_att_attr_apply_gather", "vqa_att_attr_apply_gather_f16", "vqa_att_attr_score_grouped",
                    "vqa_att_attr_score_grouped_pairs", "vqa_att_attr_score_grouped_f16", "vqa_att_attr_score_grouped_pairs_f16",
                    "vqa_att_attr_score_grouped_path")


# ----------------------------------------------------------------------------- the identity, in float64


@pytest.mark.parametrize("G", [1, 2])
@pytest.mark.parametrize("do_option", ["+", "*", "|"])
def test_closed_form_equals_autograd_in_float64(do_option, G):
    sd, vn, qf, img, answers, grid = _random_case(do_option, G, seed=10 * G + R.MODES[do_option])
    ref = R.autograd_reference(sd, do_option, vn, qf, img, answers, grid)
    got = R.closed_form(*R.model_inputs(sd, do_option, vn, qf, img, answers))
    scale = float(ref.abs().max())
    err = float((got["R"] - ref).abs().max()) / scale
    print(f"[identity] '{do_option}' G={G}: closed form vs autograd {err:.3e} of max|ref| = {scale:.3e}, "
          f"max|r1| {float(got['r1'].abs().max()):.3e}, max|r2| {float(got['r2'].abs().max()):.3e}")
    assert scale > 0 and float(got["r2"].abs().max()) > 0          # both paths carry something
    assert err < 1e-10
    # the two halves the kernels compute, from the same pieces
    half = R.closed_form_from_probs(vn, got["probs"], R.model_inputs(sd, do_option, vn, qf, img, answers)[5], img)
    assert torch.equal(half["r1"], got["r1"]) and torch.equal(half["dscore"], got["dscore"])
    args = R.model_inputs(sd, do_option, vn, qf, img, answers)
    assert float((R.score_half(got["r1"], got["dscore"], args[1], args[2], args[3], img, args[7]) - got["R"]).abs().max()) \
        < 1e-12 * scale


def test_the_logits_of_the_reference_are_the_oracles():
    """forward64 / autograd_reference run the oracle's own attention and classifier: on a fixture their logits are
    vqa_forward's (float64 against the stored fp32 logits of the reference)."""
    f = R.fixture_case("+")
    logits = R.forward64(f["golden"].sd, "+", f["vn"], f["qf"], f["img"], f["grid"])
    own = [b for b, (i, j) in enumerate(zip(R.IMAGE_INDEX, R.QUESTION_SEL)) if i == j]     # the fixture's own pairs
    assert own
    for b in own:
        assert float((logits[b].float() - f["golden"].t["logits"][R.IMAGE_INDEX[b]]).abs().max()) < 1e-5


# ----------------------------------------------------------------------------- the sign-flip condition of the GPU fixtures
@pytest.mark.parametrize("do_option", ["+", "*", "|"])
def test_no_pre_activation_of_the_gpu_fixtures_is_within_rounding_of_zero(do_option):
    """The indicators s = [. > 0] are discontinuous: tests/test_attribution_gpu.py compares fp32 maps with this float64
    reference on the golden fixtures, which only means something where no ReLU pre-activation of the asked pairs lies
    within 1e-5 * max|.| of zero.  If this fails for a fixture, other pairs have to be asked of it -- the count stays zero."""
    f = R.fixture_case(do_option)
    answers = [0] * len(R.IMAGE_INDEX)
    _, vp, qp, _, _, _, img, mode = R.model_inputs(f["golden"].sd, do_option, f["vn"], f["qf"], f["img"], answers)
    n = R.near_zero_count(vp, qp, img, mode)
    print(f"[sign-flip] {R.FIXTURES[do_option]}: {n} of {len(img) * vp.shape[1] * vp.shape[2]} pre-activations within "
          f"{R.NEAR_ZERO:g} * max of zero")
    assert n == 0


# ----------------------------------------------------------------------------- the ABI
def test_new_entry_points_in_header_prototypes_and_library():
    from dl_vqa_amd import _lib, build
    build.build_library(verbose=False)
    with open(_lib.HEADER_PATH) as f:
        header = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    for name in NEW_ENTRY_POINTS:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in _lib.PROTOTYPES, name
    lib = _lib.load()
    assert lib.vqa_abi_version() == _lib.header_abi_version() == 9          # appended, not bumped
    for name in NEW_ENTRY_POINTS:
        assert hasattr(lib, name), name


def test_attr_apply_gather_argument_validation_without_gpu():
    """dout, dout_ld, probs, vn, img, dscore, dscore_rowsum, r1, N, B, P, C, G, stream: vqa_att_apply_gather_dscore's checks
    plus r1 (pointers are made-up aligned integers: every check runs on the host before any HIP call)."""
    from dl_vqa_amd import _lib
    lib = _lib.load()
    err = lib.vqa_last_error
    for f, half in ((lib.vqa_att_attr_apply_gather, False), (lib.vqa_att_attr_apply_gather_f16, True)):
        assert f(16, 64, 16, 16, 16, 16, 16, None, 2, 3, 4, 8, 2, None) == 1 and b"null pointer" in err()      # no r1
        assert f(16, 64, 16, 16, None, 16, 16, 16, 2, 3, 4, 8, 2, None) == 1 and b"img" in err()
        assert f(16, 64, 16, 16, 16, 16, 16, 16, 2, 3, 4, 8, 9, None) == 1 and b"glimpses" in err()
        assert f(16, 64, 16, 16, 16, 16, 16, 16, 2, 3, 4, 6, 2, None) == 1 and b"multiple of 4" in err()       # C = 6
        assert f(16, 8, 16, 16, 16, 16, 16, 16, 2, 3, 4, 8, 2, None) == 1 and b"dout_ld" in err()              # dout_ld < G*C
        assert f(20, 64, 16, 16, 16, 16, 16, 16, 2, 3, 4, 8, 2, None) == 1 and b"aligned" in err()             # dout
        assert f(16, 64, 16, 20, 16, 16, 16, 16, 2, 3, 4, 8, 2, None) == 1 and b"aligned" in err()             # vn at 4 (mod 8)
        assert (f(16, 64, 16, 24, 16, 16, 16, 16, 2, 0, 4, 8, 2, None) == 0) == half                           # vn at 8 (mod 16)
        assert f(16, 64, 16, 16, 16, 16, None, 16, 2, 0, 4, 8, 2, None) == 0                                   # B = 0, no rowsum


def test_attr_score_grouped_argument_validation_without_gpu():
    """r1, dscore, vprime, qp, [qrow,] wx, wx_ld, order, offsets, out, N, B, [M,] P, mid, G, mode, stream: the grouped
    forward's checks (att_score_check) on the new operands."""
    from dl_vqa_amd import _lib
    lib = _lib.load()
    err = lib.vqa_last_error
    for f in (lib.vqa_att_attr_score_grouped, lib.vqa_att_attr_score_grouped_f16):
        assert f(16, 16, 16, 16, 16, 8, 16, 16, 16, 2, 3, 4, 8, 9, 0, None) == 1 and b"glimpses" in err()
        assert f(16, 16, 16, 16, 16, 8, 16, 16, 16, 2, 3, 4, 6, 2, 0, None) == 1 and b"mid=6" in err()
        assert f(16, 16, 16, 16, 16, 8, None, 16, 16, 2, 3, 4, 8, 2, 0, None) == 1 and b"order" in err()
        assert f(16, 16, 16, 16, 16, 8, 16, 16, 16, 2, 3, 4, 8, 2, 3, None) == 1 and b"mode 3" in err()
        assert f(None, 16, 16, 16, 16, 8, 16, 16, 16, 2, 3, 4, 8, 2, 0, None) == 1 and b"null pointer" in err()   # r1
        assert f(16, None, 16, 16, 16, 8, 16, 16, 16, 2, 3, 4, 8, 2, 0, None) == 1 and b"null pointer" in err()   # dscore
        assert f(16, 16, 16, None, 16, 8, 16, 16, 16, 2, 3, 4, 8, 2, 0, None) == 1 and b"null pointer" in err()   # '+' needs q'
        assert f(16, 16, 16, None, 16, 16, 16, 16, 16, 2, 0, 4, 8, 2, 2, None) == 0                               # '|' does not
        assert f(16, 16, 16, 16, 16, 8, 16, 16, 16, 2, 3, 4, 8, 2, 2, None) == 1 and b"wx_ld" in err()            # '|': wx_ld < 2 mid
        assert f(16, 16, 16, 16, 16, 8192, 16, 16, 16, 2, 3, 4, 8192, 2, 0, None) == 1 and b"LDS" in err()
        assert f(16, 16, 20, 16, 16, 8, 16, 16, 16, 2, 3, 4, 8, 2, 0, None) == 1 and b"aligned" in err()          # vprime
        assert f(16, 16, 16, 16, 16, 8, 16, 16, 16, 0, 3, 4, 8, 2, 0, None) == 1 and b"out of range" in err()     # N = 0
        assert f(16, 16, 16, 16, 16, 8, 16, 16, 16, 2, 0, 4, 8, 2, 0, None) == 0                                  # B = 0
    for f in (lib.vqa_att_attr_score_grouped_pairs, lib.vqa_att_attr_score_grouped_pairs_f16):
        assert f(16, 16, 16, 16, None, 16, 8, 16, 16, 16, 2, 3, 5, 4, 8, 2, 0, None) == 1 and b"qrow" in err()
        assert f(16, 16, 16, 16, 16, 16, 8, 16, 16, 16, 2, 3, 0, 4, 8, 2, 0, None) == 1 and b"M=0" in err()
        assert f(16, 16, 16, 16, 16, 16, 8, 16, 16, 16, 2, 3, 5, 4, 8, 9, 0, None) == 1 and b"glimpses" in err()
        assert f(16, 16, 16, 16, 16, 16, 8, 16, 16, 16, 2, 0, 5, 4, 8, 2, 0, None) == 0
    # the path the launcher takes: the grouped forward's (0: the register kernel, else positions per wave)
    path = lib.vqa_att_attr_score_grouped_path
    assert [path(0, 256), path(1, 1024), path(2, 256), path(0, 24), path(0, 1028), path(1, 2048), path(0, 2052)] == \
        [0, 0, 4, 4, 2, 2, 1]


# ----------------------------------------------------------------------------- the result type
# (what explain / explain_pairs refuse before any device work: tests/test_explain_refusals_cpu.py)
def test_attribution_fields():
    assert Attribution._fields == ("maps", "answers", "logits")
