"""What the tests of the explain family share (test_attribution_*, test_word_attribution_*, test_occlusion_*,
test_word_occlusion_*, test_integrated_*, test_explain_refusals_cpu and the other refusal tests): the tiny model, host-side
caches, the scripted call and the random float64 case of the CPU tests, and the model builder,
groupings, error measures and given answer columns of the GPU tests.  A plain module: no fixture, no pytest setting."""
import torch

from dl_vqa_amd import ImageFeatures, QuestionFeatures, VqaNet
from tests import attribution_ref as R
from tests.golden_util import Golden, tiny_cfg

DEV = "cuda:0"


# ----------------------------------------------------------------------------- CPU: a model and caches that never see a device
def tiny():
    g = Golden("tiny_plus")
    m = VqaNet(tiny_cfg(g.meta), g.meta["V"])
    m.load_state_dict(g.sd)
    return g, m


def host_caches(m, N=3, M=2, vprime=True):
    """Holders as encode_images / encode_questions build them, around host tensors (vprime=False: a bank without v')."""
    eng = m._engine
    m._flat_param = torch.zeros(4)
    feats = ImageFeatures(torch.zeros(N, 4, eng.C), torch.zeros(N * 4, eng.mid) if vprime else None, (2, 2), m)
    qfeats = QuestionFeatures(torch.zeros(M, eng.Q), torch.zeros(M, eng.mid), m)
    return feats, qfeats


GOOD_MAPS = torch.zeros(3, 2, 2)    # for three questions on host_caches' 2 x 2 grid: nothing about these maps is wrong


def invoke(m, name, pairs, feats, qfeats, q, ql, index, maps=None, **kw):
    """One explain call about three questions on host caches: the pairs forms ask the questions [0, 1, 1] of qfeats.  maps: the
    argument the faithfulness calls take behind the index."""
    own = () if maps is None else (maps,)
    if pairs:
        return getattr(m, name)(feats, qfeats, index, [0, 1, 1], *own, **kw)
    return getattr(m, name)(feats, q, ql, index, *own, **kw)


def columns(B, A):
    """The given answer columns of the tests."""
    return [(3 * b + 1) % A for b in range(B)]


def _random_case(do_option, G, seed):
    """A random attention stage + classifier in float64 (state-dict names and shapes of the model) and random inputs."""
    g = torch.Generator().manual_seed(seed)
    N, B, gh, gw, C, mid, Q, hid, A = 3, 7, 3, 4, 10, 12, 6, 9, 5
    xld = 2 * mid if do_option == "|" else mid
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    sd = {"attention.v_conv.weight": rn(mid, C, 1, 1), "attention.q_lin.weight": rn(mid, Q), "attention.q_lin.bias": rn(mid),
          "attention.x_conv.weight": rn(G, xld, 1, 1), "attention.x_conv.bias": rn(G),
          "classifier.lin1.weight": rn(hid, G * C + Q), "classifier.lin1.bias": rn(hid),
          "classifier.lin2.weight": rn(A, hid), "classifier.lin2.bias": rn(A)}
    vn = rn(N, gh * gw, C)
    vn = vn / vn.norm(dim=-1, keepdim=True)
    qf = rn(B, Q)
    img = torch.randint(0, N, (B,), generator=g)
    answers = torch.randint(0, A, (B,), generator=g)
    return sd, vn, qf, img, answers, (gh, gw)


# ----------------------------------------------------------------------------- GPU
def rel(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-30)


def within(tag, got, ref, bound, label):
    e = float((got.double().cpu() - ref.double().cpu()).abs().max())
    print(f"[{label}] {tag}: max|diff| = {e:.3e} (bound {bound:.3e}), max|ref| = {float(ref.abs().max()):.3e}")
    assert e <= bound, f"{tag}: {e} > {bound}"
    return e


def build(cfg, V, sd=None, compute_dtype="fp32"):
    m = VqaNet(cfg, V, compute_dtype=compute_dtype)
    if sd is not None:
        m.load_state_dict(sd)
    return m.to(DEV)


def fixture_model(do_option, compute_dtype="fp32"):
    f = R.fixture_case(do_option)
    g = f["golden"]
    m = build(f["cfg"], g.meta["V"], g.sd, compute_dtype).eval()
    return f, m, m.encode_images(f["v"].to(DEV))


def grouping(kind, N, B, g):
    """tests/test_multi_question_gpu.py's groupings, restated."""
    if kind == "empty":          # image N-1 (and, for N > 2, image 1) has no question; every other one has some
        pool = [n for n in range(N) if n != N - 1 and (N <= 2 or n != 1)]
        return torch.tensor(pool)[torch.randint(0, len(pool), (B,), generator=g)]
    if kind == "single":         # one image holds every question
        return torch.full((B,), N // 2, dtype=torch.int64)
    return torch.randint(0, N, (B,), generator=g)      # shuffled


def off_by_one_float(t):
    """The same values at an address that is 4 (mod 16): forces the scalar form."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view
