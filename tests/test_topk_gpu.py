"""GPU: top-k answers with probabilities (vqa_softmax_topk, dl_vqa_amd.topk_answers, VqaNet.predict) against the stable-sort
reference of tests/topk_ref.py (pinned by tests/test_topk_ref_cpu.py).

Indices are compared exactly.  Probabilities against float64: relative error of every returned probability <= 4e-6 --
(|x - max| + log2 A + 8) * 2^-24 with |x - max| <= 20 by construction and A <= 3073 is 2.4e-6, with headroom for expf's
last ulps; lse within 1e-5 absolute."""
import functools

import pytest
import torch

from tests.golden_util import Golden, tiny_cfg
from tests.test_shared_train_gpu import IMAGE_INDEX, _fixture_batch
from tests.topk_ref import topk_reference

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (B, A, ld, k, offset of the view in its buffer, in floats)
SHAPES = [(1, 1, 1, 1, 0),
          (3, 12, 12, 12, 0),                 # k == A
          (7, 65, 72, 3, 1),                  # rows are not 16-byte aligned; two columns per lane
          (2, 257, 257, 32, 0),
          (5, 1000, 1000, 5, 0),
          (4, 3000, 3004, 10, 0),
          (300, 24, 24, 1, 0),                # more rows than one grid wave of four-row workgroups
          (2, 64, 64, 64, 0),
          # the sizes at which the row changes its register form (64 / 256 / 1024 / 3072 columns) and the first one past the
          # last of them, where the row is re-read through the cache instead
          (2, 256, 256, 4, 0), (1, 1024, 1024, 3, 0), (1, 1025, 1025, 3, 0), (1, 3072, 3072, 3, 0), (2, 3073, 3076, 7, 3)]
IDS = ["x".join(map(str, s[:4])) for s in SHAPES]
GUARD = 64
SENT_I, SENT_F = -7777, 1234.5
PROB_RTOL, LSE_ATOL = 4e-6, 1e-5


def _gen(shape, kind):
    return torch.Generator().manual_seed(sum(p * s for p, s in zip((1009, 17, 3, 131), shape[:4])) + kind)


@functools.lru_cache(maxsize=None)
def inputs(shape, kind):
    """kind 'a': randn * 3 clamped to +-10, rows with pairwise distinct entries: a row in which two entries meet (both
    clamped onto the same bound, or the same fp32 value drawn twice) is drawn again, and distinctness is asserted;
    'b': integers from [-3, 3], massive ties."""
    B, A = shape[:2]
    if kind == "a":
        g = _gen(shape, 1)
        x = torch.empty(B, A)
        for b in range(B):
            for _ in range(100):
                x[b] = (torch.randn(A, generator=g) * 3).clamp(-10, 10)
                if x[b].unique().numel() == A:
                    break
            assert x[b].unique().numel() == A, "the entries of a row must be pairwise distinct"
        assert float(x.abs().max()) <= 10
        return x
    return torch.randint(-3, 4, (B, A), generator=_gen(shape, 2)).float()


@functools.lru_cache(maxsize=None)
def reference(shape, kind):
    return topk_reference(inputs(shape, kind), shape[3])


def device_view(x, ld, off):
    """x [B, A] as a view with row stride ld that starts `off` floats into its buffer."""
    B, A = x.shape
    buf = torch.full((off + B * ld,), 99.0, device=DEV)
    view = buf[off:off + B * ld].view(B, ld)[:, :A]
    view.copy_(x)
    return view


def run_guarded(view, k):
    """The entry point itself on outputs that sit between guard regions filled with a sentinel: (idx, prob, lse) and the
    assertion that nothing outside [B][k] / [B] changed."""
    from dl_vqa_amd import _lib
    B, A = view.shape
    ld = view.stride(0) if B > 1 else A
    idx = torch.full((2 * GUARD + B * k,), SENT_I, dtype=torch.int32, device=DEV)
    prob = torch.full((2 * GUARD + B * k,), SENT_F, device=DEV)
    lse = torch.full((2 * GUARD + B,), SENT_F, device=DEV)
    _lib.call("vqa_softmax_topk", view.data_ptr(), ld, B, A, k, idx[GUARD:].data_ptr(), prob[GUARD:].data_ptr(),
              lse[GUARD:].data_ptr(), _lib.stream())
    torch.cuda.synchronize()
    for t, n, s in ((idx, B * k, SENT_I), (prob, B * k, SENT_F), (lse, B, SENT_F)):
        assert bool((t[:GUARD] == s).all()) and bool((t[GUARD + n:] == s).all()), "a write outside the output"
    return idx[GUARD:GUARD + B * k].view(B, k).cpu(), prob[GUARD:GUARD + B * k].view(B, k).cpu(), lse[GUARD:GUARD + B].cpu()


def check_probs(tag, prob, lse, want_prob, want_lse):
    rel = float(((prob.double() - want_prob).abs() / want_prob).max())
    dl = float((lse.double() - want_lse).abs().max())
    print(f"[topk] {tag}: max rel err of a probability {rel:.3e} (tol {PROB_RTOL:.0e}), max |lse err| {dl:.3e} (tol {LSE_ATOL:.0e})")
    assert rel <= PROB_RTOL and dl <= LSE_ATOL


@pytest.mark.parametrize("kind", ["a", "b"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_kernel_matches_the_stable_sort_reference(shape, kind):
    from dl_vqa_amd import ops
    B, A, ld, k, off = shape
    x = inputs(shape, kind)
    want_idx, want_prob, want_lse = reference(shape, kind)
    view = device_view(x, ld, off)
    assert off == 0 or view.data_ptr() % 16 != 0
    idx, prob, lse = run_guarded(view, k)
    assert idx.dtype == torch.int32 and torch.equal(idx.long(), want_idx)
    check_probs(f"{shape} {kind}", prob, lse, want_prob, want_lse)
    # the tensor-level wrapper on the same view: the same bits, twice; without lse the same picks
    i1, p1, l1 = ops.softmax_topk(view, k, want_lse=True)
    i2, p2 = ops.softmax_topk(view, k)
    torch.cuda.synchronize()
    assert torch.equal(i1.cpu(), idx) and torch.equal(p1.cpu(), prob) and torch.equal(l1.cpu(), lse)
    assert torch.equal(i2, i1) and torch.equal(p2, p1)
    assert bool((view.cpu() == x).all())                                 # the input is read only


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_signed_zeros_are_equal_and_ranked_by_column(shape):
    """Row 0: negative values, one 1.0 and a handful of zeros of alternating sign spread over the row -- fewer zeros than k
    where k allows, so the picks span them: 1.0 first, then every zero by column whatever its sign."""
    B, A, ld, k, off = shape
    x = inputs(shape, "a").clone()
    x[0] = -1.0 - x[0].abs()
    nz = max(1, min(A, k) - 2)
    cols = torch.linspace(0, A - 1, nz).round().long().unique()
    x[0, cols] = torch.tensor([-0.0, 0.0] * len(cols))[:len(cols)]
    if A > len(cols):
        free = [c for c in range(A - 1, -1, -1) if c not in set(cols.tolist())]
        x[0, free[0]] = 1.0
    assert bool(torch.signbit(x[0, cols[0]])) and float(x[0, cols[0]]) == 0.0
    want_idx, want_prob, want_lse = topk_reference(x, k)
    idx, prob, lse = run_guarded(device_view(x, ld, off), k)
    assert torch.equal(idx.long(), want_idx)
    zeros_picked = [c for c in idx[0].tolist() if float(x[0, c]) == 0.0]
    assert zeros_picked == sorted(zeros_picked) and len(zeros_picked) == min(len(cols), k - (A > len(cols)))
    check_probs(f"{shape} zeros", prob, lse, want_prob, want_lse)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_nan_row(shape):
    """The last row holds two NaNs (one where A == 1): they come first, by column; that row's probabilities and lse are NaN;
    every other row has the bits it has without them."""
    B, A, ld, k, off = shape
    x = inputs(shape, "a").clone()
    x[B - 1, A - 1] = float("nan")
    x[B - 1, A // 3] = -float("nan")
    want_idx, _, _ = topk_reference(x, k)
    idx, prob, lse = run_guarded(device_view(x, ld, off), k)
    assert torch.equal(idx.long(), want_idx)
    assert idx[B - 1, 0] == A // 3 and (k == 1 or A == 1 or idx[B - 1, 1] == A - 1)
    assert bool(torch.isnan(prob[B - 1]).all()) and bool(torch.isnan(lse[B - 1]))
    idx0, prob0, lse0 = run_guarded(device_view(inputs(shape, "a"), ld, off), k)
    assert torch.equal(idx[:B - 1], idx0[:B - 1]) and torch.equal(prob[:B - 1], prob0[:B - 1]) and torch.equal(lse[:B - 1], lse0[:B - 1])


def test_empty_batch():
    from dl_vqa_amd import ops, topk_answers
    idx, prob, lse = ops.softmax_topk(torch.empty(0, 24, device=DEV), 5, want_lse=True)
    assert idx.shape == (0, 5) and idx.dtype == torch.int32 and prob.shape == (0, 5) and lse.shape == (0,)
    top = topk_answers(torch.empty(0, 24, device=DEV), 5)
    assert top.indices.shape == (0, 5) and top.indices.dtype == torch.int64 and top.probs.shape == (0, 5)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_top1_is_the_answer_the_score_kernel_scores(shape):
    """Massive ties (input b), every answer listed (a_idx[b] = 1..A) with a random count: the VQA score of the loss head is
    the sum over the rows of min(1, 0.3 * count of topk_answers' first pick).  The expected rows are summed by the
    reduction the loss head uses, so the two sums have the same terms in the same order."""
    from dl_vqa_amd import ops, topk_answers
    from dl_vqa_amd.train import soft_ce_loss_and_score
    B, A = shape[:2]
    logits = inputs(shape, "b").to(DEV)
    a_idx = torch.arange(1, A + 1).repeat(B, 1)
    a_val = torch.randint(0, 11, (B, A), generator=_gen(shape, 3))
    _, score = soft_ce_loss_and_score(logits, a_idx.to(DEV), a_val.to(DEV))
    top = topk_answers(logits, 1)
    assert top.indices.dtype == torch.int64 and top.indices.shape == (B, 1)
    assert torch.equal(top.indices.cpu()[:, 0], logits.cpu().max(dim=1).indices)       # torch.max: the first maximum
    rows = torch.clamp(torch.gather(a_val.to(DEV), 1, top.indices).float()[:, 0] * 0.3, max=1.0)
    want = torch.empty(1, device=DEV)
    ops.colsum(rows.contiguous(), B, 1, want)
    diff = abs(float(score) - float(want))
    print(f"[topk] {shape} score {float(score):.6f}, from top-1 {float(want):.6f}, |diff| {diff:.1e}")
    assert diff <= 1e-6


def test_topk_answers_on_other_dtypes_and_layouts():
    from dl_vqa_amd import topk_answers
    x = inputs(SHAPES[3], "a")                                           # [2, 257]
    want = topk_answers(x.to(DEV), 4)
    assert not want.indices.requires_grad and not want.probs.requires_grad and want.probs.dtype == torch.float32
    got = topk_answers(x.double().to(DEV), 4)                            # widened with .float(): x is exact in fp32
    assert torch.equal(got.indices, want.indices) and torch.equal(got.probs, want.probs)
    got = topk_answers(x.t().contiguous().to(DEV).t(), 4)                # column-major: copied to rows
    assert torch.equal(got.indices, want.indices) and torch.equal(got.probs, want.probs)
    half = topk_answers(x.half().to(DEV), 4)
    assert torch.equal(half.indices.cpu(), topk_reference(x.half().float(), 4)[0])


# ----------------------------------------------------------------------------- the whole path
def _tiny():
    from tests.test_model_gpu import build
    g = Golden("tiny_plus")
    cfg = tiny_cfg(g.meta)
    m = build(cfg, g.meta["V"], g.sd).eval()
    v, q, ql, _, _ = _fixture_batch(g)
    return g, m, v.to(DEV), q.to(DEV), ql.to(DEV)


def test_predict_is_answer_followed_by_the_kernel():
    from dl_vqa_amd import TopAnswers, topk_answers
    g, m, v, q, ql = _tiny()
    feats = m.encode_images(v)
    logits, att = m.answer(feats, q, ql, IMAGE_INDEX, return_attention=True)
    assert logits.shape == (7, 12)
    want = topk_answers(logits, 3)
    m._ensure_flat()
    flat_grad = m._flat_grad
    flat_grad.fill_(3.0)
    torch.manual_seed(77)
    rng = torch.get_rng_state()
    top = m.predict(feats, q, ql, IMAGE_INDEX, k=3)
    top2, att2 = m.predict(feats, q, ql, IMAGE_INDEX.tolist(), k=3, return_attention=True)
    torch.cuda.synchronize()
    assert isinstance(top, TopAnswers) and top.indices.shape == (7, 3) and top.indices.dtype == torch.int64
    assert torch.equal(top.indices, want.indices) and torch.equal(top.probs, want.probs)
    assert torch.equal(top2.indices, want.indices) and torch.equal(top2.probs, want.probs) and torch.equal(att2, att)
    ref_idx, ref_prob, _ = topk_reference(logits.cpu(), 3)
    assert torch.equal(top.indices.cpu(), ref_idx)
    assert float(((top.probs.cpu().double() - ref_prob).abs() / ref_prob).max()) <= PROB_RTOL
    # nothing kept, nothing drawn
    assert m._last_ctx is None and len(m._pending) == 0
    assert m._flat_grad is flat_grad and bool((flat_grad == 3.0).all())
    assert torch.equal(torch.get_rng_state(), rng)
    assert all(p.grad is None for p in m.parameters())
    flat_grad.zero_()
    # no questions: empty [0, k]
    e, ea = m.predict(feats, q[:0], ql[:0], [], k=3, return_attention=True)
    assert e.indices.shape == (0, 3) and e.indices.dtype == torch.int64 and e.probs.shape == (0, 3) and ea.shape[0] == 0
    # answer() itself is what it was
    assert torch.equal(m.answer(feats, q, ql, IMAGE_INDEX), logits)


def test_topk_answers_leaves_a_pending_backward_usable():
    from dl_vqa_amd import topk_answers
    g, m, v, q, ql = _tiny()
    vq = v[IMAGE_INDEX]
    y_ref = m(vq, q, ql)
    torch.autograd.backward(y_ref, torch.ones_like(y_ref))
    want = {k: p.grad.clone() for k, p in m.named_parameters()}
    for p in m.parameters():
        p.grad = None
    y = m(vq, q, ql)
    assert y.requires_grad
    top = topk_answers(y, 1)
    assert not top.indices.requires_grad and not top.probs.requires_grad and top.probs.grad_fn is None
    assert torch.equal(top.indices.cpu(), topk_reference(y.detach().cpu(), 1)[0])
    torch.autograd.backward(y, torch.ones_like(y))
    torch.cuda.synchronize()
    for k, p in m.named_parameters():
        assert torch.equal(p.grad, want[k]), k
    # forward_shared's logits are ranked alike
    with torch.no_grad():
        ys = m.forward_shared(v, q, ql, IMAGE_INDEX)
    assert torch.equal(topk_answers(ys, 2).indices.cpu(), topk_reference(ys.cpu(), 2)[0])
