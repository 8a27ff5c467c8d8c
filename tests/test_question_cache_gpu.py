"""GPU: cached question features -- vqa_att_score_grouped_pairs_fwd against the existing grouped kernel (bit for bit) and
against float64, vqa_gather_rows against src[rows], and VqaNet.encode_questions / answer_pairs / predict_pairs against
answer() on the expanded questions, the stored reference logits and the CPU oracle."""
import pytest
import torch

from dl_vqa_amd import group_by_image, topk_answers, unique_questions
from tests.golden_util import TINY_CASES, Golden, full_cfg, tiny_cfg
from tests.test_kernels_gpu import check
from tests.test_multi_question_gpu import _full224, build, rel, score_reference

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (N, B, M, P, mid, G), modes: the general kernel with P < tile; the register fast path at IT = 1 with a tile tail
# (37 = 2 * 16 + 5) and at IT = 4; the general kernel with 2 positions per wave (mid = 2048)
SCORE_SHAPES = [((3, 7, 2, 4, 24, 2), (0, 1, 2)), ((2, 9, 3, 37, 256, 1), (0, 1)), ((2, 5, 4, 20, 1024, 2), (0, 1)),
                ((2, 6, 3, 9, 2048, 3), (0,))]
SCORE_CASES = [(shape, mode) for shape, modes in SCORE_SHAPES for mode in modes]
GROUPINGS = ["shuffled", "empty", "one_question"]


def _ops():
    from dl_vqa_amd import ops
    return ops


def _score_inputs(shape, mode, kind):
    """Host inputs of one score case: a shuffled image per pair (`order` is then no identity), with `empty` one image nobody
    asks about, with `one_question` every pair on the same question row."""
    N, B, M, P, mid, G = shape
    g = torch.Generator().manual_seed(N * 1000 + B * 100 + M * 10 + mode)
    vp = torch.randn(N * P, mid, generator=g)
    qp_u = torch.randn(M, mid, generator=g)
    wx = torch.randn(G, 2 * mid if mode == 2 else mid, generator=g)
    bx = torch.randn(G, generator=g)
    if kind == "empty":
        img = torch.randint(0, N - 1, (B,), generator=g)              # image N-1 has no pair
    else:
        img = torch.arange(B).flip(0) % N                             # every image asked about, pairs interleaved: `order`
        assert img.tolist() != sorted(img.tolist())                   # is no identity
    qrow = torch.full((B,), M - 1, dtype=torch.int64) if kind == "one_question" else torch.randint(0, M, (B,), generator=g)
    return vp, qp_u, wx, bx, img, qrow


def _run_pairs(shape, mode, kind):
    ops = _ops()
    N, B, M, P, mid, G = shape
    vp, qp_u, wx, bx, img, qrow = _score_inputs(shape, mode, kind)
    order, offsets = group_by_image(img, N)
    d = lambda t: t.to(DEV)
    got = ops.att_score_grouped_pairs_fwd(d(vp), d(qp_u), d(qrow.to(torch.int32)), d(wx), d(bx), d(order), d(offsets),
                                          N, B, P, mode)
    torch.cuda.synchronize()
    assert got.shape == (B, G, P)
    return got, (vp, qp_u, wx, bx, img, qrow, order, offsets)


# ----------------------------------------------------------------------------- the pairs kernel
@pytest.mark.parametrize("kind", GROUPINGS)
@pytest.mark.parametrize("shape,mode", SCORE_CASES)
def test_pairs_score_equals_the_grouped_kernel_on_expanded_rows(shape, mode, kind):
    ops = _ops()
    N, B, M, P, mid, G = shape
    got, (vp, qp_u, wx, bx, img, qrow, order, offsets) = _run_pairs(shape, mode, kind)
    d = lambda t: t.to(DEV)
    want = ops.att_score_grouped_fwd(d(vp), d(qp_u[qrow].contiguous()), d(wx), d(bx), d(order), d(offsets), N, B, P, mode)
    torch.cuda.synchronize()
    assert torch.equal(got, want), float((got - want).abs().max())


@pytest.mark.parametrize("kind", GROUPINGS)
@pytest.mark.parametrize("shape,mode", SCORE_CASES)
def test_pairs_score_matches_float64(shape, mode, kind):
    """The bound is test_grouped_score_matches_float64's (tests/test_multi_question_gpu.py): 3e-6 of the largest score."""
    N, B, M, P, mid, G = shape
    got, (vp, qp_u, wx, bx, img, qrow, _, _) = _run_pairs(shape, mode, kind)
    want = score_reference(vp, qp_u[qrow], wx, bx, img, P, mode)
    check(f"att_score_grouped_pairs {shape} mode {mode} {kind}", got, want, 3e-6)


def test_pairs_score_skips_a_question_row_out_of_range():
    """A qrow entry outside [0, M) leaves that pair's score row unwritten and reads nothing (both kernels)."""
    ops = _ops()
    for shape, mode in (((2, 5, 3, 20, 256, 2), 0), ((2, 5, 3, 5, 24, 2), 2)):
        N, B, M, P, mid, G = shape
        vp, qp_u, wx, bx, img, qrow = _score_inputs(shape, mode, "shuffled")
        order, offsets = group_by_image(img, N)
        d = lambda t: t.to(DEV)
        good = ops.att_score_grouped_pairs_fwd(d(vp), d(qp_u), d(qrow.to(torch.int32)), d(wx), d(bx), d(order), d(offsets),
                                               N, B, P, mode)
        bad = qrow.clone()
        bad[1], bad[3] = M, -1
        from dl_vqa_amd._lib import call, ptr, stream
        score = torch.full((B, G, P), 7.0, device=DEV)
        dev = [d(vp), d(qp_u), d(bad.to(torch.int32)), d(wx), d(bx), d(order), d(offsets)]
        call("vqa_att_score_grouped_pairs_fwd", ptr(dev[0]), ptr(dev[1]), ptr(dev[2]), ptr(dev[3]), wx.shape[1], ptr(dev[4]),
             ptr(dev[5]), ptr(dev[6]), ptr(score), N, B, M, P, mid, G, mode, stream())
        torch.cuda.synchronize()
        keep = torch.tensor([b not in (1, 3) for b in range(B)], device=DEV)
        assert torch.equal(score[keep], good[keep])
        assert bool((score[~keep] == 7.0).all())


# ----------------------------------------------------------------------------- vqa_gather_rows
@pytest.mark.parametrize("B,M,cols,src_pad,dst_off,dst_pad", [
    (5, 3, 4, 0, 0, 0),            # one float4 per row
    (7, 4, 20, 12, 8, 4),          # vector path, both sides strided (a column range of a wider buffer)
    (1, 3, 64, 0, 4, 0),           # B == 1
    (300, 9, 2048, 0, 512, 0),     # the classifier input's shape: more than one block
    (6, 4, 20, 0, 3, 2),           # dst column offset 3: 12-byte aligned, the scalar path
    (6, 4, 18, 1, 0, 0),           # cols and src_ld no multiple of 4: the scalar path
])
def test_gather_rows_equals_indexing(B, M, cols, src_pad, dst_off, dst_pad):
    ops = _ops()
    g = torch.Generator().manual_seed(B * 100 + cols)
    src_buf = torch.randn(M, cols + src_pad, generator=g).to(DEV)
    src = src_buf[:, :cols]
    rows = torch.randint(0, M, (B,), generator=g)
    if B > 2:
        rows[2] = rows[0]                                             # a repeated row index
    dst_buf = torch.full((B, dst_off + cols + dst_pad), 7.0, device=DEV)
    dst = dst_buf[:, dst_off:dst_off + cols]
    ops.gather_rows(src, rows.to(torch.int32).to(DEV), dst, cols)
    torch.cuda.synchronize()
    assert torch.equal(dst, src[rows.to(DEV)])
    assert bool((dst_buf[:, :dst_off] == 7.0).all()) and bool((dst_buf[:, dst_off + cols:] == 7.0).all())


def test_gather_rows_writes_zeros_for_a_row_out_of_range():
    ops = _ops()
    for cols in (8, 6):                                               # vector and scalar path
        src = torch.randn(3, cols, generator=torch.Generator().manual_seed(cols)).to(DEV)
        rows = torch.tensor([2, 3, 0, -1], dtype=torch.int32, device=DEV)
        dst = torch.full((4, cols), 7.0, device=DEV)
        ops.gather_rows(src, rows, dst, cols)
        torch.cuda.synchronize()
        assert torch.equal(dst[0], src[2]) and torch.equal(dst[2], src[0])
        assert bool((dst[1] == 0).all()) and bool((dst[3] == 0).all())


# ----------------------------------------------------------------------------- the whole path on the fixtures
IMG = torch.tensor([0, 1, 2, 2, 0, 1, 1])          # test_answer_matches_reference_and_oracle_on_fixtures' pairs: rows 0-2
QSEL = torch.tensor([0, 1, 2, 0, 1, 2, 1])         # are the fixture's own (image, question) pairs


@pytest.mark.parametrize("name", TINY_CASES)
def test_answer_pairs_matches_answer_reference_and_oracle_on_fixtures(name):
    from oracle import vqa_oracle as O
    g = Golden(name)
    cfg = tiny_cfg(g.meta)
    m = build(cfg, g.meta["V"], g.sd).eval()
    v, q, ql = g.t["v"], g.t["q"], g.t["q_len"]
    q_u, ql_u, first = unique_questions(q[:3], ql[:3])
    qidx = first[QSEL]
    assert torch.equal(ql_u[qidx], ql[QSEL])
    feats = m.encode_images(v[:3].to(DEV))
    qfeats = m.encode_questions(q_u.to(DEV), ql_u.to(DEV))
    assert qfeats.M == q_u.shape[0] and qfeats.qf.shape == (qfeats.M, m._engine.Q)
    assert qfeats.qprime.shape == (qfeats.M, cfg["attention"]["hidden_dim"]) and not qfeats.qprime.requires_grad
    logits, att = m.answer_pairs(feats, qfeats, IMG, qidx, return_attention=True)
    y_ans, a_ans = m.answer(feats, q_u[qidx].to(DEV), ql_u[qidx].to(DEV), IMG, return_attention=True)
    torch.cuda.synchronize()
    gh, gw = feats.grid
    assert logits.shape == (7, cfg["max_answers"]) and att.shape == (7, 2, gh, gw)
    assert not logits.requires_grad and not att.requires_grad
    e_ans = float((logits - y_ans).abs().max())
    e_att = rel(att.reshape(7, 2, -1), a_ans.reshape(7, 2, -1))
    e_ref = float((logits[:3].cpu() - g.t["logits"][:3]).abs().max())
    y_or = O.vqa_forward(g.sd, cfg, v[IMG], q[QSEL], ql[QSEL])
    e_or = float((logits.cpu() - y_or).abs().max())
    print(f"[question-cache] {name}: logits vs answer {e_ans:.3e}, attention rel {e_att:.3e}, vs reference {e_ref:.3e}, "
          f"vs oracle {e_or:.3e}")
    assert e_ans < 1e-5
    assert e_att < 2e-5
    assert e_ref < 1e-5
    assert e_or < 1e-5
    assert float((att.sum(dim=(2, 3)) - 1).abs().max()) < 1e-5


# ----------------------------------------------------------------------------- north-star architecture
@pytest.mark.parametrize("compute_dtype", ["fp32", "fp32x3"])
def test_answer_pairs_full224(compute_dtype):
    """2 images, 3 distinct questions, 6 pairs against answer(); bounds of test_answer_full224_reference_and_oracle
    (1e-3 on the logits; the stored reference logits for the fixture's own two pairs)."""
    g, m, v, q, ql = _full224(compute_dtype)
    q3 = torch.cat([q, q[:1]])                        # a third question: question 0 cut to another length
    ql3 = torch.cat([ql, torch.clamp(ql[:1] - 2, min=1)])
    q_u, ql_u, first = unique_questions(q3, ql3)
    assert q_u.shape[0] == 3
    img = torch.tensor([0, 1, 1, 0, 0, 1])
    qidx = torch.tensor([0, 1, 0, 2, 1, 2])
    feats = m.encode_images(v.to(DEV))
    qfeats = m.encode_questions(q_u.to(DEV), ql_u.to(DEV))
    logits, att = m.answer_pairs(feats, qfeats, img, qidx, return_attention=True)
    y_ans, a_ans = m.answer(feats, q_u[qidx].to(DEV), ql_u[qidx].to(DEV), img, return_attention=True)
    torch.cuda.synchronize()
    e_ans = float((logits - y_ans).abs().max())
    e_att = rel(att.reshape(6, 2, -1), a_ans.reshape(6, 2, -1))
    e_ref = float((logits[:2].cpu() - g.t["logits"]).abs().max())
    print(f"[question-cache] full224 ({compute_dtype}): logits vs answer {e_ans:.3e}, attention rel {e_att:.3e}, "
          f"vs reference {e_ref:.3e}")
    assert e_ans < 1e-3
    assert e_att < 1e-4
    assert e_ref < 1e-3
    assert m._last_ctx is None


# ----------------------------------------------------------------------------- order invariance, bit for bit
def test_order_invariance_of_pairs_and_of_question_rows():
    from oracle import vqa_oracle as O
    V, N, M, B, T = 500, 5, 11, 48, 9
    torch.manual_seed(9)
    m = build(full_cfg(100), V).eval()
    v, q, _, _, _, _, ql = O.synthetic_batch(max(N, M), 64, T, V, 100, seed=11)
    feats = m.encode_images(v[:N].to(DEV))
    q_u, ql_u, _ = unique_questions(q[:M], ql[:M])
    assert q_u.shape[0] == M
    qfeats = m.encode_questions(q_u.to(DEV), ql_u.to(DEV))
    gen = torch.Generator().manual_seed(12)
    img = torch.randint(0, N, (B,), generator=gen)
    qidx = torch.randint(0, M, (B,), generator=gen)
    y0, a0 = m.answer_pairs(feats, qfeats, img, qidx, return_attention=True)
    # permuting the pairs permutes the rows
    perm = torch.randperm(B, generator=gen)
    y1, a1 = m.answer_pairs(feats, qfeats, img[perm], qidx[perm], return_attention=True)
    torch.cuda.synchronize()
    assert torch.equal(y1, y0[perm.to(DEV)]) and torch.equal(a1, a0[perm.to(DEV)])
    # permuting the rows of q_u with question_index remapped leaves every pair as it was
    rp = torch.randperm(M, generator=gen)             # new row j holds old row rp[j]
    inv = torch.empty_like(rp)
    inv[rp] = torch.arange(M)
    qfeats2 = m.encode_questions(q_u[rp].to(DEV), ql_u[rp].to(DEV))
    y2 = m.answer_pairs(feats, qfeats2, img, inv[qidx])
    # CUDA indices (one synchronising copy each) and plain lists give the same rows
    y3 = m.answer_pairs(feats, qfeats, img.to(DEV), qidx.tolist())
    torch.cuda.synchronize()
    assert torch.equal(y2, y0)
    assert torch.equal(y3, y0)
    # predict_pairs is answer_pairs + topk_answers
    for k in (1, 5):
        top = m.predict_pairs(feats, qfeats, img, qidx, k=k)
        want = topk_answers(y0, k)
        assert torch.equal(top.indices, want.indices) and torch.equal(top.probs, want.probs)
    top, a5 = m.predict_pairs(feats, qfeats, img, qidx, k=5, return_attention=True)
    assert torch.equal(a5, a0) and top.indices.shape == (B, 5)
    # empty requests
    y_e, a_e = m.answer_pairs(feats, qfeats, [], [], return_attention=True)
    assert y_e.shape == (0, 100) and a_e.shape == (0, 2) + feats.grid
    q_e = m.encode_questions(torch.zeros(0, T, dtype=torch.int64), torch.zeros(0, dtype=torch.int64))
    assert q_e.M == 0 and q_e.qf.shape == (0, m._engine.Q) and q_e.qprime.shape == (0, 1024)
    assert m.answer_pairs(feats, q_e, [], []).shape == (0, 100)
    with pytest.raises(IndexError):
        m.answer_pairs(feats, q_e, [0], [0])


# ----------------------------------------------------------------------------- existing behaviour untouched, ownership
def test_forward_backward_unchanged_after_the_new_calls_and_ownership():
    from dl_vqa_amd.train import soft_ce_loss_and_score
    g = Golden("tiny_plus")
    cfg = tiny_cfg(g.meta)
    v, q, ql = g.t["v"].to(DEV), g.t["q"].to(DEV), g.t["q_len"].to(DEV)
    a_idx, a_val = g.t["a_idx"].to(DEV), g.t["a_val"].to(DEV)
    B = q.shape[0]

    def step(m):
        y = m(v, q, ql)
        soft_ce_loss_and_score(y, a_idx, a_val)[0].backward()
        torch.cuda.synchronize()
        return y.detach().clone(), {k: p.grad.clone() for k, p in m.named_parameters()}

    fresh = build(cfg, g.meta["V"], g.sd).train()
    torch.manual_seed(21)
    y_f, g_f = step(fresh)

    m = build(cfg, g.meta["V"], g.sd).eval()
    m._ensure_flat()
    flat_grad = m._flat_grad
    flat_grad.fill_(3.0)
    torch.manual_seed(77)
    rng = torch.get_rng_state()
    feats = m.encode_images(v)
    qfeats = m.encode_questions(q, ql)
    y_a = m.answer_pairs(feats, qfeats, [(b + 1) % feats.N for b in range(B)], list(range(B)))
    top = m.predict_pairs(feats, qfeats, [0] * B, list(range(B)), k=2)
    torch.cuda.synchronize()
    assert m._last_ctx is None and len(m._pending) == 0
    assert m._flat_grad is flat_grad and bool((flat_grad == 3.0).all())
    assert torch.equal(torch.get_rng_state(), rng)                  # the dropout seed stream was not drawn from
    assert all(p.grad is None for p in m.parameters())
    assert y_a.shape == y_f.shape and top.indices.shape == (B, 2)
    flat_grad.zero_()
    m.train()
    torch.manual_seed(21)                                           # the seeded train step of the fresh model
    y_m, g_m = step(m)
    assert torch.equal(y_m, y_f)
    for k in g_f:
        assert torch.equal(g_m[k], g_f[k]), k
    m.eval()
    fresh.eval()

    # question features of another model instance are refused; so are those of a model that was moved / re-flattened since
    with pytest.raises(RuntimeError, match="question features belong elsewhere"):
        fresh.answer_pairs(fresh.encode_images(v), qfeats, [0] * B, list(range(B)))
    with pytest.raises(RuntimeError, match="image features belong elsewhere"):
        fresh.answer_pairs(feats, fresh.encode_questions(q, ql), [0] * B, list(range(B)))
    m.to("cpu")
    m.to(DEV)                                                       # new parameter storage
    f2 = m.encode_images(v)
    with pytest.raises(RuntimeError, match="question features belong elsewhere"):
        m.answer_pairs(f2, qfeats, [0] * B, list(range(B)))
    qf2 = m.encode_questions(q, ql)
    assert torch.equal(m.answer_pairs(f2, qf2, [(b + 1) % feats.N for b in range(B)], list(range(B))), y_a)
    # errors raised before any launch
    with pytest.raises(IndexError):
        m.encode_questions(torch.full_like(q, g.meta["V"]).cpu(), ql)
    with pytest.raises(RuntimeError, match="question length"):
        m.encode_questions(q, torch.zeros_like(ql).cpu())
    # a device token id >= V is counted by the embedding kernel and surfaces at check_token_ids()
    m.check_token_ids()
    bad = q.clone()
    bad[0, 0] = g.meta["V"]
    m.encode_questions(bad, ql)
    with pytest.raises(IndexError, match="out of range"):
        m.check_token_ids()
    m.check_token_ids()                                             # reported once
