"""CPU: per-token gradient x input (VqaNet.explain_words) -- the closed forms of the two new kernels in float64 against autograd
through the oracle's pieces (tests/word_attribution_ref.py), the '|' identity, the conditions under which the GPU tests on the
fixtures and on the random fused-recurrence models are meaningful, the new entry points in the header, the ctypes prototypes
and the built library with their host-side argument validation.  (The errors the public call raises before any device work:
tests/test_explain_refusals_cpu.py.)"""
import re

import pytest
import torch

from dl_vqa_amd import VqaNet, WordAttribution
from tests import attribution_ref as R
from tests import word_attribution_ref as W

NEW_ENTRY_POINTS = ("vqa_att_attr_dq_grouped", "vqa_att_attr_dq_grouped_f16", "vqa_embed_attr")


# ----------------------------------------------------------------------------- the closed forms, in float64
@pytest.mark.parametrize("do_option", ["+", "*", "|"])
def test_closed_forms_of_steps_3_and_7_equal_autograd_in_float64(do_option):
    f = R.fixture_case(do_option)
    sd = f["golden"].sd
    answers = W.fixture_argmax(do_option)
    full, att, cls = W.fixture_reference(do_option, answers)
    scale = float(full["words"].abs().max())
    assert scale > 0
    # the two variants are the two paths: they add up to the whole
    assert float((att["words"] + cls["words"] - full["words"]).abs().max()) < 1e-12 * scale
    # step 3: d logit / d q' through the scores, from the dscore of the map's closed form
    args = R.model_inputs(sd, do_option, f["vn"], full["qf"], f["img"], answers)
    _vn, vp, qp, wx, _bx, _dwv, img, mode = args
    dscore = R.closed_form(*args)["dscore"]
    dq = W.dq_closed_form(dscore, vp, qp, wx, img, mode)
    dq_scale = max(float(att["dqp"].abs().max()), float(full["dqp"].abs().max()))
    e3 = float((dq - att["dqp"]).abs().max())
    # the classifier does not read q', so the full graph's gradient at q' is the attention path's
    assert float((full["dqp"] - att["dqp"]).abs().max()) <= 1e-12 * max(dq_scale, 1e-300)
    # step 7: the embedding stage, from the gradient at x = tanh(e)
    e7 = 0.0
    for part in (full, att, cls):
        wc = W.words_closed_form(sd["text.embedding.weight"], f["q"], part["x"], part["dx"], f["q_len"])
        e7 = max(e7, float((wc - part["words"]).abs().max()))
    share = float(att["words"].abs().max()) / scale
    print(f"[identity-words] '{do_option}': max|words| {scale:.3e}, attention path's share {share:.3e}, step 3 closed form vs "
          f"autograd {e3:.3e} of max|dq'| {dq_scale:.3e}, step 7 {e7:.3e}")
    if mode != 2:
        assert dq_scale > 0 and share > 0                           # the attention path carries something
        assert e3 < 1e-12 * dq_scale
    assert e7 < 1e-12 * scale
    # padded slots are exactly zero, in the reference too
    T = f["q"].shape[1]
    pad = torch.arange(T)[None, :] >= f["q_len"][:, None]
    assert bool(pad.any()) and bool((full["words"][pad] == 0).all())
    # a faithful fp32 evaluation of the same graph, for scale: what the GPU bound has to leave room for
    f32 = W.autograd_reference(sd, do_option, f["vn"], f["q"], f["q_len"], f["img"], answers, f["grid"],
                               f["cfg"]["text"]["bidirectional"], dtype=torch.float32)
    e32 = float((f32["words"].double() - full["words"]).abs().max()) / scale
    print(f"[identity-words] '{do_option}': fp32 CPU evaluation of the same graph off float64 by {e32:.3e} of the maximum")
    assert e32 < 2e-5


def test_the_attention_path_of_cat_is_identically_zero():
    """'|': the q' half adds the same constant to every position's score and softmax is shift-invariant, so nothing behind the
    softmax depends on q' through the scores.  The closed form the engine follows (no kernel, no q_lin product) IS zero.
    Autograd does not know the identity: it sums p * (t - sum p t) over the positions in floating point and is left with the
    rounding of that sum -- measured 9.5e-19 at q' (where the other fixtures hold 2.6e-4 and 1.9e-5) and 3.8e-18 of
    max|words| -- so the autograd variant is asserted zero to within 1e-15 of the maximum, not bit for bit."""
    f = R.fixture_case("|")
    answers = W.fixture_argmax("|")
    full, att, _cls = W.fixture_reference("|", answers)
    args = R.model_inputs(f["golden"].sd, "|", f["vn"], full["qf"], f["img"], answers)
    dq = W.dq_closed_form(R.closed_form(*args)["dscore"], args[1], args[2], args[3], args[6], args[7])
    assert args[7] == 2 and bool((dq == 0).all())                   # exactly
    scale = float(full["words"].abs().max())
    print(f"[identity-words] '|' attention-only by autograd: max|words| {float(att['words'].abs().max()):.3e} of {scale:.3e}, "
          f"max|dq'| {float(att['dqp'].abs().max()):.3e}")
    assert float(att["words"].abs().max()) <= 1e-15 * scale
    assert float(att["dqp"].abs().max()) <= 1e-15
    # and the score rows do carry a gradient: the zero is the identity's, not an empty graph's
    assert float(R.closed_form(*args)["dscore"].abs().max()) > 0


@pytest.mark.parametrize("do_option", ["+", "*", "|"])
def test_no_pre_activation_of_the_fixtures_is_within_rounding_of_zero(do_option):
    """The ReLU indicators are discontinuous: the GPU tests compare fp32 results with this float64 reference, which only
    means something where no pre-activation of the asked pairs lies within 1e-5 * max|.| of zero."""
    assert W.case_near_zero(R.fixture_case(do_option), do_option) == 0


@pytest.mark.parametrize("bidirectional", [True, False])
def test_the_random_fused_recurrence_models_are_clear_of_zero_too(bidirectional):
    """tests/test_word_attribution_gpu.py item 4: a seeded random model with H = 32.  The seed (word_attribution_ref.RANDOM_SEED)
    was chosen here, on the CPU, so that the count is zero; T = 6 and T = 1."""
    for T in (6, 1):
        case = W.random_case(bidirectional, T)
        assert case["cfg"]["text"]["question_features"] == 32 and case["q"].shape == (5, T)
        assert sorted(case["q_len"].tolist())[0] == 1 and int(case["q_len"].max()) == T
        assert W.case_near_zero(case, "+") == 0


# ----------------------------------------------------------------------------- the ABI
def test_new_entry_points_in_header_prototypes_and_library():
    from dl_vqa_amd import _lib, build
    build.build_library(verbose=False)
    with open(_lib.HEADER_PATH) as f:
        text = f.read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW_ENTRY_POINTS:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in _lib.PROTOTYPES, name
        assert name in text.split("#define VQA_ABI_VERSION")[0], name      # listed among the append-only additions
    lib = _lib.load()
    assert lib.vqa_abi_version() == _lib.header_abi_version() == 9          # appended, not bumped
    for name in NEW_ENTRY_POINTS:
        assert hasattr(lib, name), name
    # declared with the other attribution entry points, behind them
    order = re.findall(r"\b(vqa_[a-z0-9_]+)\s*\(", header)
    at = order.index("vqa_att_attr_score_grouped_pairs_f16")
    assert tuple(order[at + 1:at + 4]) == NEW_ENTRY_POINTS


def test_attr_dq_grouped_argument_validation_without_gpu():
    """dscore, vprime, qp, wx, wx_ld, order, offsets, dq_part, N, B, P, mid, G, mode, stream (pointers are made-up aligned
    integers: every check runs on the host before any HIP call)."""
    from dl_vqa_amd import _lib
    lib = _lib.load()
    err = lib.vqa_last_error
    for f, half in ((lib.vqa_att_attr_dq_grouped, False), (lib.vqa_att_attr_dq_grouped_f16, True)):
        assert f(16, 16, 16, 16, 8, 16, 16, 16, 2, 3, 4, 8, 2, 2, None) == 1
        assert b"shift-invariant" in err() and b"identically zero" in err()                                # '|' says why
        assert f(16, 16, 16, 16, 8, 16, 16, 16, 2, 3, 4, 8, 2, 3, None) == 1 and b"mode 3" in err()
        assert f(16, 16, 16, 16, 8, 16, 16, 16, 2, 3, 4, 8, 9, 0, None) == 1 and b"glimpses" in err()
        assert f(16, 16, 16, 16, 8, 16, 16, 16, 2, 3, 4, 6, 2, 0, None) == 1 and b"mid=6" in err()
        assert f(16, 16, 16, 16, 8, None, 16, 16, 2, 3, 4, 8, 2, 0, None) == 1 and b"order" in err()
        for k in (0, 1, 2, 3, 7):                                                                            # every data pointer
            a = [16, 16, 16, 16, 8, 16, 16, 16, 2, 3, 4, 8, 2, 1, None]
            a[k] = None
            assert f(*a) == 1 and b"null pointer" in err(), k
        assert f(16, 16, 16, 16, 8192, 16, 16, 16, 2, 3, 4, 8192, 2, 0, None) == 1 and b"mid=8192" in err()
        assert f(16, 20, 16, 16, 8, 16, 16, 16, 2, 3, 4, 8, 2, 0, None) == 1 and b"aligned" in err()        # vprime at 4 (mod 8)
        assert (f(16, 24, 16, 16, 8, 16, 16, 16, 2, 0, 4, 8, 2, 0, None) == 0) == half                      # vprime at 8 (mod 16)
        assert f(16, 16, 16, 16, 8, 16, 16, 24, 2, 3, 4, 8, 2, 0, None) == 1 and b"aligned" in err()        # dq_part
        assert f(16, 16, 16, 16, 8, 16, 16, 16, 0, 3, 4, 8, 2, 0, None) == 1 and b"out of range" in err()   # N = 0
        assert f(16, 16, 16, 16, 8, 16, 16, 16, 2, 0, 4, 8, 2, 1, None) == 0                                # B = 0: no launch


def test_embed_attr_argument_validation_without_gpu():
    """q, emb, x, dx0, dx1, q_len, words, B, T, E, V, stream."""
    from dl_vqa_amd import _lib
    lib = _lib.load()
    err = lib.vqa_last_error
    f = lib.vqa_embed_attr
    for k in (0, 1, 2, 3, 5, 6):
        a = [16, 16, 16, 16, 16, 16, 16, 3, 4, 8, 10, None]
        a[k] = None
        assert f(*a) == 1 and b"null pointer" in err(), k
    assert f(16, 16, 16, 16, 16, 16, 16, -1, 4, 8, 10, None) == 1 and b"out of range" in err()
    assert f(16, 16, 16, 16, 16, 16, 16, 3, 0, 8, 10, None) == 1 and b"out of range" in err()
    assert f(16, 16, 16, 16, 16, 16, 16, 3, 4, 0, 10, None) == 1 and b"out of range" in err()
    assert f(16, 16, 16, 16, 16, 16, 16, 3, 4, 8, 0, None) == 1 and b"out of range" in err()
    assert f(16, 16, 16, 16, None, 16, 16, 0, 4, 8, 10, None) == 0          # B = 0: no launch; dx1 may be NULL
    assert f(16, 20, 16, 16, 16, 16, 16, 0, 4, 7, 10, None) == 0            # no alignment or width rule: the scalar form


# ----------------------------------------------------------------------------- the result type and the missing pairs form
# (what explain_words refuses before any device work: tests/test_explain_refusals_cpu.py)
def test_word_attribution_is_exported():
    import dl_vqa_amd
    assert "WordAttribution" in dl_vqa_amd.__all__ and dl_vqa_amd.WordAttribution is WordAttribution
    assert WordAttribution._fields == ("words", "maps", "answers", "logits")
    assert not hasattr(VqaNet, "explain_words_pairs")                # QuestionFeatures holds no recurrence state
    assert "no explain_words_pairs" in VqaNet.explain_words.__doc__
