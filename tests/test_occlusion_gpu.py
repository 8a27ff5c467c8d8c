"""GPU: occlusion maps from cached features -- vqa_occl_logit against float64 (tests/occlusion_ref.py) on synthetic inputs,
and VqaNet.explain_occlusion / explain_occlusion_pairs on the golden fixtures against the brute-force route on the device
(answer() on caches with the occluded rows zeroed) and against the float64 brute force, with the bit-for-bit relations to
answer, explain, a widened float16 cache and a permuted batch."""
import functools
import math

import pytest
import torch

from dl_vqa_amd import ImageFeatures, Occlusion, unique_questions
from tests import attribution_ref as R
from tests import occlusion_ref as OR
from tests.explain_util import columns as _columns, fixture_model as _fixture_model, grouping as _grouping, within
from tests.test_kernels_gpu import check

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_within = functools.partial(within, label="parity-occlusion")
ALPHA_MAX = 16.0          # the numerical contract of vqa_occl_logit (include/vqa_hip.h)


def _ops():
    from dl_vqa_amd import ops
    return ops


# ----------------------------------------------------------------------------- the kernel against float64
# (B, R, gh, gw, G, hid, window): one position (the denominator is r alone); a window larger than the grid; hid of one and of
# several quads per lane, with and without a tail; every window; G = 1..4; 26 x 26 positions (more than one chunk per wave)
SHAPES = [(3, 2, 1, 1, 1, 20, 1), (4, 3, 2, 2, 2, 20, 3), (3, 2, 5, 7, 2, 1024, 1), (3, 2, 5, 7, 4, 520, 3),
          (2, 2, 5, 7, 3, 1028, 5), (2, 1, 3, 4, 2, 256, 7)]
LARGE = (2, 2, 26, 26, 2, 1024, 3)
A = 11


def _case(shape, kind):
    """Consistent synthetic operands of vqa_occl_logit: probs = softmax(score), Z = sum_p probs * U in float64, rounded.
    cnull = the row's log-sum-exp + log r with r drawn so that alpha = 1 / (1 - mass + |S| * r) stays inside the contract: a
    window that can hold the whole attention mass leaves the denominator |S| * r alone, so r is near 1 there (cnull near the
    log-sum-exp); otherwise the denominator is at least r, drawn from [1/15, 0.6], hence alpha <= 15 whatever the mass.  So
    that the comparison also reaches the far side of the contract, question 0 of those cases has r = 1/15 and one position
    that holds nearly all of its attention mass (alpha about 10 there)."""
    B, Rr, gh, gw, G, hid, window = shape
    P = gh * gw
    g = torch.Generator().manual_seed(1000 * B + 100 * gh + 10 * G + window)
    slot = _grouping(kind, Rr, B, g) if Rr > 1 else torch.zeros(B, dtype=torch.int64)      # one image: one grouping
    score = 2 * torch.randn(B, G, P, generator=g)
    whole = 2 * (window // 2) >= max(gh, gw) - 1                  # some S(p) is the whole grid
    if not whole:
        score[0, :, P // 2] += 5 + math.log(P)
    probs = torch.softmax(score, dim=-1)
    U = torch.randn(Rr, P, G, hid, generator=g)
    Z = torch.einsum("bgp,bpgh->bgh", probs.double(), U.double()[slot]).float()
    base = torch.randn(B, hid, generator=g)
    lo, hi = (0.6, 1.4) if whole else (1.0 / 15.0, 0.6)
    r = torch.exp(math.log(lo) + (math.log(hi) - math.log(lo)) * torch.rand(B, G, generator=g))
    if not whole:
        r[0] = lo
    cnull = (torch.logsumexp(score.double(), -1) + torch.log(r.double())).float()
    W2 = torch.randn(A, hid + 4, generator=g)                     # leading dimensions wider than the rows
    logits = torch.randn(B, A + 1, generator=g)
    b2 = torch.randn(A, generator=g)
    answers = torch.randint(0, A, (B,), generator=g)
    return dict(base=base, Z=Z, U=U, slot=slot, probs=probs, score=score, cnull=cnull, W2=W2, b2=b2, answers=answers,
                logits=logits, grid=(gh, gw), window=window)


def _run(c, perm=None, answers=None, out=None):
    ops = _ops()
    hid = c["base"].shape[1]
    d = lambda t: (t if perm is None else t[perm]).to(DEV)
    cols = c["answers"] if answers is None else answers
    return ops.occl_logit(d(c["base"]), d(c["Z"]), c["U"].to(DEV), d(c["slot"]).to(torch.int32), d(c["probs"]), d(c["score"]),
                          d(c["cnull"]), c["W2"].to(DEV)[:, :hid], c["b2"].to(DEV), d(cols).to(torch.int32),
                          d(c["logits"])[:, :A], *c["grid"], c["window"], out=out)


def _check_kernel(shape, kind):
    c = _case(shape, kind)
    B = shape[0]
    hid = c["base"].shape[1]
    ref = OR.kernel_form(c["base"], c["Z"], c["U"], c["slot"], c["probs"], c["score"], c["cnull"], c["W2"][:, :hid], c["b2"],
                         c["answers"], c["grid"], c["window"])
    amax = float(ref["alpha"].max())
    print(f"[parity-occlusion] {shape} {kind}: alpha in [{float(ref['alpha'].min()):.3f}, {amax:.3f}], max mass "
          f"{float(ref['mass'].max()):.4f}")
    assert 0 < float(ref["alpha"].min()) and amax <= ALPHA_MAX      # every (b, g, p) compared is inside the contract
    maps = _run(c)
    torch.cuda.synchronize()
    logit = c["logits"][:, :A].gather(1, c["answers"][:, None]).double()
    check(f"occl_logit {shape} {kind}", logit - maps.double().cpu(), ref["occluded"], 3e-6)
    # permuting the questions permutes the rows, bit for bit
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(5))
    assert torch.equal(_run(c, perm=perm), maps[perm.to(DEV)])
    # a column out of range gives a zero row and leaves the others as they were
    bad = c["answers"].clone()
    bad[0], bad[B - 1] = A, -1
    zero = _run(c, answers=bad, out=torch.full_like(maps, 7.0))
    assert float(zero[0].abs().max()) == 0.0 and float(zero[B - 1].abs().max()) == 0.0
    assert torch.equal(zero[1:B - 1], maps[1:B - 1])
    return c, maps


@pytest.mark.parametrize("kind", ["empty", "single", "shuffled"])
@pytest.mark.parametrize("shape", SHAPES)
def test_occl_logit_matches_float64(shape, kind):
    _check_kernel(shape, kind)


def test_occl_logit_matches_float64_on_a_26_x_26_grid():
    c, maps = _check_kernel(LARGE, "shuffled")
    # U in chunks of images: a question whose row is not in the chunk is left alone, and the two calls write every row once
    ops = _ops()
    hid = c["base"].shape[1]
    d = lambda t: t.to(DEV)
    out = torch.full_like(maps, 7.0)
    for r0 in (0, 1):
        ops.occl_logit(d(c["base"]), d(c["Z"]), d(c["U"][r0:r0 + 1]), d(c["slot"]).to(torch.int32), d(c["probs"]), d(c["score"]),
                       d(c["cnull"]), d(c["W2"])[:, :hid], d(c["b2"]), d(c["answers"]).to(torch.int32), d(c["logits"])[:, :A],
                       *c["grid"], c["window"], slot0=r0, out=out)
        if r0 == 0:
            assert bool((out[d(c["slot"]) == 1] == 7.0).all())
    assert torch.equal(out, maps)


def test_occl_logit_refuses_a_width_that_is_no_multiple_of_4():
    from dl_vqa_amd._lib import VqaHipError
    c = _case((3, 2, 2, 2, 1, 18, 1), "shuffled")
    with pytest.raises(VqaHipError, match="multiple of 4"):
        _run(c)
    for window in (0, 2, 9):
        with pytest.raises(VqaHipError, match="window"):
            _run({**_case((3, 2, 2, 2, 1, 20, 1), "shuffled"), "window": window})


# ----------------------------------------------------------------------------- the whole path on the golden fixtures
MODELS = [("+", "fp32"), ("*", "fp32"), ("|", "fp32"), ("+", "fp32x3"), ("*", "fp32x3"), ("|", "fp32x3")]


@functools.lru_cache(maxsize=None)
def _fixture_run(do_option, compute_dtype):
    """One fixture in one compute mode: the model, its caches, answer() on the full caches and on the four caches with one
    position's rows zeroed in vn and in v' (the brute-force route), each computed once."""
    f, m, feats = _fixture_model(do_option, compute_dtype)
    q, ql, img = f["q"].to(DEV), f["q_len"].to(DEV), list(R.IMAGE_INDEX)
    N, P, _ = feats.vn.shape
    full = m.answer(feats, q, ql, img)
    occluded = []
    for p in range(P):
        vn, vp = feats.vn.clone(), feats.vprime.clone()
        vn[:, p, :] = 0
        vp.view(N, P, -1)[:, p, :] = 0
        occluded.append(m.answer(ImageFeatures(vn, vp, feats.grid, m), q, ql, img))
    torch.cuda.synchronize()
    return dict(f=f, m=m, feats=feats, q=q, ql=ql, img=img, full=full, occluded=torch.stack(occluded, 1))      # [B, P, A]


def _picked(t, cols):
    """t[..., A] at each question's column."""
    idx = torch.as_tensor(cols, dtype=torch.int64, device=t.device)
    return t.gather(-1, idx.view(-1, *([1] * (t.dim() - 1))).expand(*t.shape[:-1], 1))[..., 0]


@functools.lru_cache(maxsize=None)
def _bound(compute_dtype):
    """The tolerance of the whole-path tests, measured on code that is not under test: the largest absolute difference, over
    the three fixtures, between answer() on the zeroed caches and the float64 brute force (the occluded logits of the
    arg-max and of the given columns), times 4 -- the closed form adds the Z - probs * U difference and one division to the
    same products, with alpha about 1 on these fixtures -- and not below 1e-7 (one ulp of a 0.27 logit is 3e-8)."""
    worst = 0.0
    for do_option in ("+", "*", "|"):
        run = _fixture_run(do_option, compute_dtype)
        f = run["f"]
        full64 = R.forward64(f["golden"].sd, do_option, f["vn"], f["qf"], f["img"], f["grid"])
        B, n_answers = full64.shape
        for cols in (run["full"].argmax(1).tolist(), _columns(B, n_answers)):
            occluded64 = _picked(full64, cols)[:, None] - OR.fixture_brute(do_option, cols, 1)
            worst = max(worst, float((_picked(run["occluded"], cols).double().cpu() - occluded64).abs().max()))
    bound = max(4 * worst, 1e-7)
    print(f"[parity-occlusion] {compute_dtype}: answer() on zeroed caches vs float64 brute force, max|diff| over the three "
          f"fixtures = {worst:.3e}; whole-path bound = max(4 x that, 1e-7) = {bound:.3e}")
    return bound


@pytest.mark.parametrize("do_option,compute_dtype", MODELS)
def test_explain_occlusion_matches_the_brute_force_route_and_float64(do_option, compute_dtype):
    run = _fixture_run(do_option, compute_dtype)
    bound = _bound(compute_dtype)
    m, feats, q, ql, img = run["m"], run["feats"], run["q"], run["ql"], run["img"]
    name = f"{R.FIXTURES[do_option]} {compute_dtype}"
    B, n_answers = run["full"].shape
    occ = m.explain_occlusion(feats, q, ql, img)
    torch.cuda.synchronize()
    assert isinstance(occ, Occlusion) and occ.maps.shape == (B, *feats.grid) and occ.maps.dtype == torch.float32
    assert occ.answers.dtype == torch.int64 and occ.answers.shape == (B,) and occ.logits.shape == (B, n_answers)
    assert not occ.maps.requires_grad and m._last_ctx is None
    # logits are answer()'s, answers are explain()'s
    assert torch.equal(occ.logits, run["full"])
    att = m.explain(feats, q, ql, img)
    assert torch.equal(occ.answers, att.answers)
    given = m.explain_occlusion(feats, q, ql, img, answers=_columns(B, n_answers))
    assert given.answers.tolist() == _columns(B, n_answers) and torch.equal(given.logits, occ.logits)
    for what, res in (("arg-max", occ), ("given columns", given)):
        cols = res.answers.tolist()
        device_brute = _picked(run["full"], cols)[:, None] - _picked(run["occluded"], cols)
        _within(f"{name} explain_occlusion {what} vs answer() on zeroed caches", res.maps.reshape(B, -1), device_brute, bound)
        _within(f"{name} explain_occlusion {what} vs float64 brute force", res.maps.reshape(B, -1),
                OR.fixture_brute(do_option, cols, 1), bound)
    # the exact map is not explain()'s first-order map
    gap = float((occ.maps - att.maps).abs().max()) / float(occ.maps.abs().max())
    print(f"[parity-occlusion] {name}: |explain_occlusion - explain| = {gap:.3f} of max|explain_occlusion|")
    assert gap > 0.05
    # window 3 on the 2 x 2 grid takes the whole image out, from every position
    w3 = m.explain_occlusion(feats, q, ql, img, answers=occ.answers, window=3)
    _within(f"{name} explain_occlusion window 3 vs float64 brute force", w3.maps.reshape(B, -1),
            OR.fixture_brute(do_option, occ.answers.tolist(), 3), bound)
    # a CUDA column out of range: a map of zeros, the other rows untouched
    bad = occ.answers.clone()
    bad[2] = n_answers
    zero = m.explain_occlusion(feats, q, ql, img, answers=bad)
    assert float(zero.maps[2].abs().max()) == 0.0 and torch.equal(zero.maps[:2], occ.maps[:2])
    assert torch.equal(zero.maps[3:], occ.maps[3:])
    # one image per chunk of U
    per_image = feats.vn.shape[1] * m._engine.G * m._engine.hid * 4
    chunked = m.explain_occlusion(feats, q, ql, img, _u_bytes=per_image)
    _within(f"{name} explain_occlusion one image per chunk vs unchunked (bit-equal: {torch.equal(chunked.maps, occ.maps)})",
            chunked.maps, occ.maps, bound)
    assert torch.equal(chunked.answers, occ.answers) and torch.equal(chunked.logits, occ.logits)
    # a permuted batch: the same rows, bit for bit
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(3))
    shuffled = m.explain_occlusion(feats, q[perm.to(DEV)], ql[perm.to(DEV)], [img[i] for i in perm.tolist()])
    assert torch.equal(shuffled.maps, occ.maps[perm.to(DEV)]) and torch.equal(shuffled.logits, occ.logits[perm.to(DEV)])
    # the same pairs from the two caches: whatever relation answer_pairs has to answer, the maps have it too
    qu, qlu, qidx = unique_questions(run["f"]["q"], run["f"]["q_len"])
    assert qu.shape[0] < B
    qfeats = m.encode_questions(qu.to(DEV), qlu.to(DEV))
    pairs = m.explain_occlusion_pairs(feats, qfeats, img, qidx)
    assert torch.equal(pairs.logits, m.answer_pairs(feats, qfeats, img, qidx))
    assert torch.equal(pairs.answers, m.explain_pairs(feats, qfeats, img, qidx).answers)
    same = torch.equal(pairs.logits, occ.logits)
    print(f"[parity-occlusion] {name}: answer_pairs logits are answer's bit for bit: {same}")
    if same:
        assert torch.equal(pairs.maps, occ.maps) and torch.equal(pairs.answers, occ.answers)
    else:
        assert float((pairs.logits - occ.logits).abs().max()) <= bound
        _within(f"{name} explain_occlusion_pairs vs explain_occlusion", pairs.maps, occ.maps, bound)
    pairs_given = m.explain_occlusion_pairs(feats, qfeats, img, qidx, answers=_columns(B, n_answers), window=3)
    _within(f"{name} explain_occlusion_pairs given columns, window 3 vs float64 brute force", pairs_given.maps.reshape(B, -1),
            OR.fixture_brute(do_option, _columns(B, n_answers), 3), bound)
    # an empty batch
    none = m.explain_occlusion(feats, q[:0], ql[:0], [])
    assert isinstance(none, Occlusion) and none.maps.shape == (0, *feats.grid) and none.logits.shape == (0, n_answers)
    none = m.explain_occlusion_pairs(feats, qfeats, [], [])
    assert none.maps.shape == (0, *feats.grid) and none.answers.dtype == torch.int64
    assert m._last_ctx is None and all(p.grad is None for p in m.parameters())


@pytest.mark.parametrize("do_option", ["+", "*", "|"])
def test_a_float16_cache_gives_what_its_widened_copy_gives(do_option):
    run = _fixture_run(do_option, "fp32")
    m, feats, q, ql, img = run["m"], run["feats"], run["q"], run["ql"], run["img"]
    f16 = feats.to(torch.float16)
    f32 = f16.to(torch.float32)
    for window in (1, 3):
        a16, a32 = m.explain_occlusion(f16, q, ql, img, window=window), m.explain_occlusion(f32, q, ql, img, window=window)
        assert torch.equal(a16.maps, a32.maps) and torch.equal(a16.logits, a32.logits) and torch.equal(a16.answers, a32.answers)
    qu, qlu, qidx = unique_questions(run["f"]["q"], run["f"]["q_len"])
    qfeats = m.encode_questions(qu.to(DEV), qlu.to(DEV))
    p16, p32 = m.explain_occlusion_pairs(f16, qfeats, img, qidx), m.explain_occlusion_pairs(f32, qfeats, img, qidx)
    assert torch.equal(p16.maps, p32.maps) and torch.equal(p16.logits, p32.logits)
    full = m.explain_occlusion(feats, q, ql, img, answers=a16.answers, window=3)
    e = float((a16.maps - full.maps).abs().max()) / float(full.maps.abs().max())
    print(f"[parity-occlusion] {R.FIXTURES[do_option]} float16 cache vs fp32 cache (window 3): maps max|diff|/max = {e:.3e}")
