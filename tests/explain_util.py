"""What the tests of the explain family share (test_attribution_*, test_word_attribution_*, test_occlusion_*,
test_word_occlusion_*, test_explain_refusals_cpu): the tiny model and host-side caches of the CPU tests, and the model builder,
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


def columns(B, A):
    """The given answer columns of the tests."""
    return [(3 * b + 1) % A for b in range(B)]


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
