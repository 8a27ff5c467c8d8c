"""CPU: integrated gradients from cached features (VqaNet.explain_integrated / explain_integrated_pairs) -- the closed form of
the path sum against autograd in float64, the condition under which the GPU tests on the golden fixtures are meaningful (no ReLU
pre-activation of the scores or of lin1 within rounding of zero anywhere on the path), completeness improving with the steps,
the new entry points in the header, the ctypes prototypes and the built library with their host-side argument validation, the
`steps` refusals and the result type."""
import re

import pytest
import torch

from dl_vqa_amd import IntegratedGradients
from dl_vqa_amd.model import integrated_alphas
from tests import attribution_ref as R
from tests import integrated_ref as I
from tests.explain_util import _random_case, host_caches, tiny

SCORE_ENTRY_POINTS = ("vqa_att_path_score_grouped", "vqa_att_path_score_grouped_pairs", "vqa_att_path_score_grouped_f16",
                      "vqa_att_path_score_grouped_pairs_f16")
ATTR_ENTRY_POINTS = ("vqa_att_path_attr_grouped", "vqa_att_path_attr_grouped_pairs", "vqa_att_path_attr_grouped_f16",
                     "vqa_att_path_attr_grouped_pairs_f16")
NEW_ENTRY_POINTS = SCORE_ENTRY_POINTS + ATTR_ENTRY_POINTS + ("vqa_att_path_scale_rows",)
GPU_FIXTURE_STEPS = (8, 16)          # what tests/test_integrated_gpu.py asks of the fixtures


# ----------------------------------------------------------------------------- the step positions
def test_the_step_positions_are_the_float32_midpoints():
    for S in (1, 3, 8, 16, 64):
        a = integrated_alphas(S)
        assert a.dtype == torch.float32 and a.shape == (S,)
        want = torch.tensor([(2 * s + 1) / (2 * S) for s in range(S)], dtype=torch.float64)
        assert torch.equal(a.double(), want.to(torch.float32).double())
        assert 0 < float(a.min()) and float(a.max()) < 1                # never alpha = 0
        assert torch.equal(I.alphas64(S), a.double())


# ----------------------------------------------------------------------------- the identity, in float64
@pytest.mark.parametrize("steps", [1, 3, 8])
@pytest.mark.parametrize("G", [1, 2])
@pytest.mark.parametrize("do_option", ["+", "*", "|"])
def test_closed_form_equals_autograd_in_float64(do_option, G, steps):
    """A random attention stage + classifier (tests/explain_util.py's), and below the three fixtures: the header's
    placement of alpha_s -- r1_s and dscore_s without it, r2_s with it -- against autograd on alpha_s * vn.  The bound is the one
    test_attribution_cpu.py has for the same comparison at alpha = 1."""
    sd, vn, qf, img, answers, grid = _random_case(do_option, G, seed=10 * G + R.MODES[do_option])
    alphas = I.alphas64(steps)
    ref = I.riemann_autograd(sd, do_option, vn, qf, img, answers, grid, alphas)
    got = I.closed_form(sd, do_option, vn, qf, img, answers, alphas)
    scale = float(ref.abs().max())
    err = float((got - ref).abs().max()) / scale
    print(f"[identity-ig] '{do_option}' G={G} S={steps}: closed form vs autograd {err:.3e} of max|ref| = {scale:.3e}")
    assert scale > 0 and err < 1e-10
    # one step at alpha = 1 is gradient x input itself
    one = I.closed_form_step(sd, do_option, vn, qf, img, answers, 1.0)
    gxi = R.closed_form(*R.model_inputs(sd, do_option, vn, qf, img, answers))
    assert float((one["G"] - gxi["R"]).abs().max()) < 1e-12 * scale
    # the two kernels' halves, from the same pieces, give the same path sum
    st = [I.closed_form_step(sd, do_option, vn, qf, img, answers, a) for a in alphas.tolist()]
    args = R.model_inputs(sd, do_option, vn, qf, img, answers)
    r1, ds = torch.stack([s["r1"] for s in st], 1), torch.stack([s["dscore"] for s in st], 1)
    halves = I.path_attr(r1, ds, args[1], args[2], args[3], img, args[7], alphas, 1.0 / steps)
    assert float((halves - got).abs().max()) < 1e-12 * scale
    sc = I.path_scores(args[1], args[2], args[3], args[4], img, args[7], alphas)
    assert float((torch.softmax(sc, -1) - torch.stack([s["probs"] for s in st], 1)).abs().max()) < 1e-12


@pytest.mark.parametrize("steps", [1, 3, 8])
@pytest.mark.parametrize("do_option", ["+", "*", "|"])
def test_closed_form_equals_autograd_on_the_fixtures(do_option, steps):
    f = R.fixture_case(do_option)
    answers = I.fixture_answers(do_option)
    alphas = I.alphas64(steps)
    ref = I.riemann_autograd(f["golden"].sd, do_option, f["vn"], f["qf"], f["img"], answers, f["grid"], alphas)
    got = I.closed_form(f["golden"].sd, do_option, f["vn"], f["qf"], f["img"], answers, alphas)
    err = float((got - ref).abs().max()) / float(ref.abs().max())
    print(f"[identity-ig] {R.FIXTURES[do_option]} S={steps}: closed form vs autograd {err:.3e} of max|ref|")
    assert err < 1e-10


# ----------------------------------------------------------------------------- the sign-flip condition of the GPU fixtures
@pytest.mark.parametrize("steps", GPU_FIXTURE_STEPS)
@pytest.mark.parametrize("do_option", ["+", "*", "|"])
def test_no_pre_activation_on_the_path_of_the_gpu_fixtures_is_within_rounding_of_zero(do_option, steps):
    """tests/test_integrated_gpu.py compares fp32 maps with the float64 Riemann sum on the golden fixtures at 8 and 16 steps,
    for the arg-max columns and for explain_util.columns: that only means something where no v' / q' pre-activation and no lin1
    pre-activation lies within 1e-5 * max|.| of zero at any step.  (At 64 steps tiny_plus has three such lin1 values: the GPU
    tests do not use 64 steps on fixtures.)"""
    from tests.explain_util import columns
    f = R.fixture_case(do_option)
    A = f["cfg"]["max_answers"]
    for answers in (I.fixture_answers(do_option), columns(len(R.IMAGE_INDEX), A)):
        n_pre, n_z = I.path_near_zero_count(f["golden"].sd, do_option, f["vn"], f["qf"], f["img"], answers, I.alphas64(steps))
        print(f"[sign-flip-ig] {R.FIXTURES[do_option]} S={steps}: {n_pre} score and {n_z} lin1 pre-activations within "
              f"{R.NEAR_ZERO:g} * max of zero")
        assert n_pre == 0 and n_z == 0


# ----------------------------------------------------------------------------- completeness
@pytest.mark.parametrize("do_option", ["+", "*", "|"])
def test_completeness_gap_falls_with_the_steps(do_option):
    """The maps sum to logit[b, a_b] - logit_at_zero_features[b, a_b] up to the quadrature error.  No absolute bound: the ReLU
    kinks make the midpoint rule first-order.  Gradient x input (the one-point rule at alpha = 1) is printed beside them."""
    f = R.fixture_case(do_option)
    sd, answers = f["golden"].sd, I.fixture_answers(do_option)
    gap = {}
    for steps in (2, 16):
        ig = I.fixture_reference(do_option, answers, steps)
        gap[steps] = float(I.fixture_gap(do_option, answers, ig).abs().max())
    gxi = R.fixture_reference(do_option, answers)[0]
    g_gxi = float(I.fixture_gap(do_option, answers, gxi).abs().max())
    cols = torch.tensor(answers)[:, None]
    rise = R.forward64(sd, do_option, f["vn"], f["qf"], f["img"], f["grid"]).gather(1, cols) - \
        R.forward64(sd, do_option, 0 * f["vn"], f["qf"], f["img"], f["grid"]).gather(1, cols)
    print(f"[completeness] {R.FIXTURES[do_option]}: max|gap| at 2 steps {gap[2]:.3e}, at 16 steps {gap[16]:.3e}, gradient x "
          f"input {g_gxi:.3e}; max|logit - logit at zero| {float(rise.abs().max()):.3e}")
    assert gap[16] < gap[2]


# ----------------------------------------------------------------------------- the ABI
def test_new_entry_points_in_header_prototypes_and_library():
    from dl_vqa_amd import _lib, build
    build.build_library(verbose=False)
    with open(_lib.HEADER_PATH) as f:
        header = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    for name in NEW_ENTRY_POINTS:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in _lib.PROTOTYPES, name
        # the prototype has as many arguments as the header's declaration
        decl = re.search(r"\b" + name + r"\s*\(([^)]*)\)", header).group(1)
        assert len(decl.split(",")) == len(_lib.PROTOTYPES[name][1]), name
    # declared behind the faithfulness entry points
    assert header.index("vqa_occl_curves(") < min(header.index(name + "(") for name in NEW_ENTRY_POINTS)
    lib = _lib.load()
    assert lib.vqa_abi_version() == _lib.header_abi_version() == 9          # appended, not bumped
    for name in NEW_ENTRY_POINTS:
        assert hasattr(lib, name), name
    assert int(re.search(r"#define\s+VQA_ATT_PATH_MAX_STEPS\s+(\d+)", header).group(1)) == 64


def test_path_score_argument_validation_without_gpu():
    """vprime, qp, [qrow,] wx, wx_ld, bx, alphas, order, offsets, score, N, B, [M,] S, P, mid, G, mode, stream: the grouped
    forward's checks (att_score_check) plus the step positions (pointers are made-up aligned integers: every check runs on the
    host before any HIP call)."""
    from dl_vqa_amd import _lib
    lib = _lib.load()
    err = lib.vqa_last_error
    for f, half in ((lib.vqa_att_path_score_grouped, False), (lib.vqa_att_path_score_grouped_f16, True)):
        assert f(16, 16, 16, 8, 16, 16, 16, 16, 16, 2, 3, 4, 5, 8, 9, 0, None) == 1 and b"glimpses" in err()
        assert f(16, 16, 16, 8, 16, 16, 16, 16, 16, 2, 3, 4, 5, 6, 2, 0, None) == 1 and b"mid=6" in err()
        assert f(16, 16, 16, 8, 16, 16, None, 16, 16, 2, 3, 4, 5, 8, 2, 0, None) == 1 and b"order" in err()
        assert f(16, 16, 16, 8, 16, 16, 16, 16, 16, 2, 3, 4, 5, 8, 2, 3, None) == 1 and b"mode 3" in err()
        assert f(16, None, 16, 8, 16, 16, 16, 16, 16, 2, 3, 4, 5, 8, 2, 0, None) == 1 and b"null pointer" in err()     # q'
        assert f(16, 16, 16, 8, None, 16, 16, 16, 16, 2, 3, 4, 5, 8, 2, 0, None) == 1 and b"null pointer" in err()     # bx
        assert f(16, 16, 16, 8, 16, 16, 16, 16, None, 2, 3, 4, 5, 8, 2, 0, None) == 1 and b"null pointer" in err()     # score
        assert f(16, 16, 16, 8, 16, None, 16, 16, 16, 2, 3, 4, 5, 8, 2, 0, None) == 1 and b"alphas" in err()
        assert f(16, 16, 16, 8, 16, 16, 16, 16, 16, 2, 3, 0, 5, 8, 2, 0, None) == 1 and b"S=0" in err()
        assert f(16, 16, 16, 8, 16, 16, 16, 16, 16, 2, 3, 65, 5, 8, 2, 0, None) == 1 and b"S=65" in err()
        assert f(16, 16, 16, 8, 16, 16, 16, 16, 16, 2, 3, 4, 5, 8, 2, 2, None) == 1 and b"wx_ld" in err()              # '|': wx_ld < 2 mid
        assert f(16, 16, 16, 8192, 16, 16, 16, 16, 16, 2, 3, 4, 5, 8192, 2, 0, None) == 1 and b"LDS" in err()
        assert f(20, 16, 16, 8, 16, 16, 16, 16, 16, 2, 3, 4, 5, 8, 2, 0, None) == 1 and b"aligned" in err()            # vprime
        assert (f(24, 16, 16, 8, 16, 16, 16, 16, 16, 2, 0, 4, 5, 8, 2, 0, None) == 0) == half                          # at 8 (mod 16)
        assert f(16, 16, 16, 8, 16, 16, 16, 16, 16, 0, 3, 4, 5, 8, 2, 0, None) == 1 and b"out of range" in err()       # N = 0
        assert f(16, 16, 16, 8, 16, 16, 16, 16, 16, 2, 0, 64, 5, 8, 2, 0, None) == 0                                   # B = 0
    for f in (lib.vqa_att_path_score_grouped_pairs, lib.vqa_att_path_score_grouped_pairs_f16):
        assert f(16, 16, None, 16, 8, 16, 16, 16, 16, 16, 2, 3, 5, 4, 5, 8, 2, 0, None) == 1 and b"qrow" in err()
        assert f(16, 16, 16, 16, 8, 16, 16, 16, 16, 16, 2, 3, 0, 4, 5, 8, 2, 0, None) == 1 and b"M=0" in err()
        assert f(16, 16, 16, 16, 8, 16, 16, 16, 16, 16, 2, 3, 5, 0, 5, 8, 2, 0, None) == 1 and b"S=0" in err()
        assert f(16, 16, 16, 16, 8, 16, 16, 16, 16, 16, 2, 3, 5, 4, 5, 8, 9, 0, None) == 1 and b"glimpses" in err()
        assert f(16, 16, 16, 16, 8, 16, 16, 16, 16, 16, 2, 0, 5, 4, 5, 8, 2, 0, None) == 0


def test_path_attr_argument_validation_without_gpu():
    """r1, dscore, vprime, qp, [qrow,] wx, wx_ld, alphas, scale, order, offsets, out, N, B, [M,] S, P, mid, G, mode, stream: the
    grouped attribution's checks plus the step positions."""
    from dl_vqa_amd import _lib
    lib = _lib.load()
    err = lib.vqa_last_error
    for f in (lib.vqa_att_path_attr_grouped, lib.vqa_att_path_attr_grouped_f16):
        assert f(16, 16, 16, 16, 16, 8, 16, 0.5, 16, 16, 16, 2, 3, 4, 5, 8, 9, 0, None) == 1 and b"glimpses" in err()
        assert f(16, 16, 16, 16, 16, 8, 16, 0.5, 16, 16, 16, 2, 3, 4, 5, 6, 2, 0, None) == 1 and b"mid=6" in err()
        assert f(16, 16, 16, 16, 16, 8, 16, 0.5, None, 16, 16, 2, 3, 4, 5, 8, 2, 0, None) == 1 and b"order" in err()
        assert f(16, 16, 16, 16, 16, 8, 16, 0.5, 16, 16, 16, 2, 3, 4, 5, 8, 2, 3, None) == 1 and b"mode 3" in err()
        assert f(None, 16, 16, 16, 16, 8, 16, 0.5, 16, 16, 16, 2, 3, 4, 5, 8, 2, 0, None) == 1 and b"null pointer" in err()   # r1
        assert f(16, None, 16, 16, 16, 8, 16, 0.5, 16, 16, 16, 2, 3, 4, 5, 8, 2, 0, None) == 1 and b"null pointer" in err()   # dscore
        assert f(16, 16, 16, None, 16, 8, 16, 0.5, 16, 16, 16, 2, 3, 4, 5, 8, 2, 0, None) == 1 and b"null pointer" in err()   # '+' needs q'
        assert f(16, 16, 16, None, 16, 16, 16, 0.5, 16, 16, 16, 2, 0, 4, 5, 8, 2, 2, None) == 0                               # '|' does not
        assert f(16, 16, 16, 16, 16, 8, None, 0.5, 16, 16, 16, 2, 3, 4, 5, 8, 2, 0, None) == 1 and b"alphas" in err()
        assert f(16, 16, 16, 16, 16, 8, 16, 0.5, 16, 16, 16, 2, 3, 0, 5, 8, 2, 0, None) == 1 and b"S=0" in err()
        assert f(16, 16, 16, 16, 16, 8, 16, 0.5, 16, 16, 16, 2, 3, 65, 5, 8, 2, 0, None) == 1 and b"S=65" in err()
        assert f(16, 16, 16, 16, 16, 8192, 16, 0.5, 16, 16, 16, 2, 3, 4, 5, 8192, 2, 0, None) == 1 and b"LDS" in err()
        assert f(16, 16, 20, 16, 16, 8, 16, 0.5, 16, 16, 16, 2, 3, 4, 5, 8, 2, 0, None) == 1 and b"aligned" in err()          # vprime
        assert f(16, 16, 16, 16, 16, 8, 16, 0.5, 16, 16, 16, 0, 3, 4, 5, 8, 2, 0, None) == 1 and b"out of range" in err()     # N = 0
        assert f(16, 16, 16, 16, 16, 8, 16, 0.5, 16, 16, 16, 2, 0, 4, 5, 8, 2, 0, None) == 0                                  # B = 0
    for f in (lib.vqa_att_path_attr_grouped_pairs, lib.vqa_att_path_attr_grouped_pairs_f16):
        assert f(16, 16, 16, 16, None, 16, 8, 16, 0.5, 16, 16, 16, 2, 3, 5, 4, 5, 8, 2, 0, None) == 1 and b"qrow" in err()
        assert f(16, 16, 16, 16, 16, 16, 8, 16, 0.5, 16, 16, 16, 2, 3, 0, 4, 5, 8, 2, 0, None) == 1 and b"M=0" in err()
        assert f(16, 16, 16, 16, 16, 16, 8, 16, 0.5, 16, 16, 16, 2, 3, 5, 65, 5, 8, 2, 0, None) == 1 and b"S=65" in err()
        assert f(16, 16, 16, 16, 16, 16, 8, 16, 0.5, 16, 16, 16, 2, 0, 5, 4, 5, 8, 2, 0, None) == 0
    # x, ld, alphas, S, rows, cols, stream
    f = lib.vqa_att_path_scale_rows
    assert f(None, 8, 16, 4, 3, 8, None) == 1 and b"null pointer" in err()
    assert f(16, 8, None, 4, 3, 8, None) == 1 and b"alphas" in err()
    assert f(16, 8, 16, 0, 3, 8, None) == 1 and b"S=0" in err()
    assert f(16, 4, 16, 4, 3, 8, None) == 1 and b"ld >= cols" in err()
    assert f(16, 8, 16, 4, 0, 8, None) == 0                                                                                   # no rows


# ----------------------------------------------------------------------------- steps, and the result type
@pytest.mark.parametrize("name,pairs", [("explain_integrated", False), ("explain_integrated_pairs", True)])
def test_steps_are_judged_before_any_device_work(name, pairs):
    g, m = tiny()
    m.eval()
    feats, qfeats = host_caches(m, N=3, M=2)
    q, ql = g.t["q"][:3], g.t["q_len"][:3]
    call = (lambda **kw: getattr(m, name)(feats, qfeats, [0, 1, 2], [0, 1, 1], **kw)) if pairs else \
        (lambda **kw: getattr(m, name)(feats, q, ql, [0, 1, 2], **kw))
    for bad in (0, 65, -1, 2.0, True, "8", None):
        with pytest.raises(ValueError, match=r"steps must be an int in 1\.\.64"):
            call(steps=bad)
    with pytest.raises(ValueError, match="steps"):                  # judged before the `answers` columns
        call(steps=0, answers=[0, 1])
    with pytest.raises(ValueError, match="2 answers for 3"):
        call(steps=8, answers=[0, 1])
    for ok in (1, 16, 64):
        with pytest.raises(RuntimeError, match="cuda"):             # everything the host can judge is in order
            call(steps=ok)
    m.train()
    with pytest.raises(RuntimeError, match="training mode"):        # judged before steps
        call(steps=0)
    assert m._last_ctx is None and all(p.grad is None for p in m.parameters())


def test_chunks_fit_the_workspace_cap():
    g, m = tiny()
    eng = m._engine
    G = eng.G
    assert eng.integrated_rows(196, 16) == (256 << 20) // (16 * 196 * (3 * G + 1) * 4)
    assert eng.integrated_rows(196, 16, ig_bytes=1) == 1            # never less than one question
    assert eng.integrated_rows(4, 8, ig_bytes=2 * 8 * 4 * (3 * G + 1) * 4) == 2


def test_integrated_gradients_fields_and_gap():
    assert IntegratedGradients._fields == ("maps", "answers", "logits", "baseline_logits")
    import dl_vqa_amd
    assert "IntegratedGradients" in dl_vqa_amd.__all__
    maps = torch.tensor([[[1.0, 2.0], [3.0, 4.0]], [[0.5, 0.0], [0.0, 0.0]]])
    out = IntegratedGradients(maps, torch.tensor([1, 0]), torch.tensor([[0.0, 9.0], [2.0, 0.0]]), torch.tensor([1.0, 0.5]))
    gap = out.completeness_gap()
    assert gap.dtype == torch.float64 and gap.tolist() == [10.0 - (9.0 - 1.0), 0.5 - (2.0 - 0.5)]
