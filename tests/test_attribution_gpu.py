"""GPU: gradient x input maps from cached features -- vqa_att_attr_apply_gather and vqa_att_attr_score_grouped against
float64 (tests/attribution_ref.py) and against the entry points whose code they share, VqaNet.explain / explain_pairs on the
golden fixtures against autograd through the oracle, order invariance bit for bit, and the existing paths untouched."""
import pytest
import torch

from dl_vqa_amd import Attribution, group_by_image, unique_questions
from tests import attribution_ref as R
from tests.explain_util import build, fixture_model as _fixture_model, grouping as _grouping, rel
from tests.golden_util import Golden, full_cfg, tiny_cfg
from tests.test_kernels_gpu import check

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _ops():
    from dl_vqa_amd import ops
    return ops


# ----------------------------------------------------------------------------- kernel 1: dscore's bits, and r1
# the apply-gather shapes of tests/test_multi_question_gpu.py.  (2, 70, 130, 3) has C % 4 != 0: the forward serves it with
# its scalar kernel, the dscore entry point refuses it, and so does this one -- its limits are the dscore entry point's;
# (2, 70, 132, 3) next to it runs the numerical checks at that size
@pytest.mark.parametrize("B,P,C,G", [(2, 70, 130, 3), (3, 100, 72, 1), (2, 17, 64, 4), (1, 65, 8, 2), (2, 676, 256, 2),
                                     (2, 70, 132, 3)])
def test_attr_apply_gather_has_dscores_bits_and_r1_matches_float64(B, P, C, G):
    from dl_vqa_amd._lib import VqaHipError
    ops = _ops()
    g = torch.Generator().manual_seed(B * 1000 + P + C)
    N, Bq = B, 2 * B + 3                                        # more questions than images, random image per question
    vn = torch.randn(N, P, C, generator=g)
    pr = torch.softmax(torch.randn(Bq, G, P, generator=g) * 2, dim=-1)
    ld = G * C + 12
    dout = torch.randn(Bq, ld, generator=g)
    img = torch.randint(0, N, (Bq,), generator=g)
    d = lambda t: t.to(DEV)
    img_d = d(img.to(torch.int32))
    if C % 4:
        for call in (ops.att_apply_gather_dscore, ops.att_attr_apply_gather):
            with pytest.raises(VqaHipError, match="multiple of 4"):
                call(d(dout), ld, d(pr), d(vn), img_d)
        return
    rs_ref, rs_new = torch.full((Bq, G), 7.0, device=DEV), torch.full((Bq, G), 9.0, device=DEV)
    ds_ref = ops.att_apply_gather_dscore(d(dout), ld, d(pr), d(vn), img_d, rowsum=rs_ref)
    ds_new, r1 = ops.att_attr_apply_gather(d(dout), ld, d(pr), d(vn), img_d, rowsum=rs_new)
    ds_nors, r1_nors = ops.att_attr_apply_gather(d(dout), ld, d(pr), d(vn), img_d)
    torch.cuda.synchronize()
    assert torch.equal(ds_new, ds_ref) and torch.equal(rs_new, rs_ref)
    assert torch.equal(ds_nors, ds_ref) and torch.equal(r1_nors, r1)
    want = R.closed_form_from_probs(vn, pr, dout[:, :G * C].reshape(Bq, G, C), img)
    check(f"att_attr_apply_gather r1 {B,P,C,G}", r1, want["r1"], 3e-6)
    check(f"att_attr_apply_gather dscore {B,P,C,G}", ds_new, want["dscore"], 1e-5)      # att_apply_gather_bwd's bound
    # a float16 vn: the fp32 form on the widened values, bit for bit
    vh = d(vn).half()
    rs16, rs32 = torch.full((Bq, G), 7.0, device=DEV), torch.full((Bq, G), 9.0, device=DEV)
    ds16, r16 = ops.att_attr_apply_gather(d(dout), ld, d(pr), vh, img_d, rowsum=rs16)
    ds32, r32 = ops.att_attr_apply_gather(d(dout), ld, d(pr), vh.float(), img_d, rowsum=rs32)
    torch.cuda.synchronize()
    assert torch.equal(ds16, ds32) and torch.equal(r16, r32) and torch.equal(rs16, rs32)
    assert torch.equal(ds16, ops.att_apply_gather_dscore(d(dout), ld, d(pr), vh, img_d))


# ----------------------------------------------------------------------------- kernel 2: R = r1 + r2
# the issue's five shapes; then mid = 768 and 512 (the register kernel's IT = 3 and 2 beside 1 and 4) and mid = 2304 (one
# position per wave), so that every branch of the launcher is reached
SCORE_SHAPES = [(3, 7, 4, 24, 2), (2, 5, 18, 256, 1), (2, 9, 33, 1024, 2), (3, 6, 20, 520, 4), (2, 5, 37, 2048, 3),
                (2, 4, 9, 768, 3), (2, 3, 5, 512, 1), (2, 4, 6, 2304, 2)]


def _expected_path(mode, mid):
    """The launcher's dispatch (csrc/att_score.hip att_score_grouped_pw), restated: 0 = the register kernel."""
    if mode != 2 and mid % 256 == 0 and mid <= 1024:
        return 0
    return 4 if mid <= 1024 else (2 if mid <= 2048 else 1)


def test_the_score_shapes_reach_every_branch_of_the_launcher():
    ops = _ops()
    reached = set()
    for (_, _, _, mid, _) in SCORE_SHAPES:
        for mode in (0, 1, 2):
            path = ops.att_attr_score_grouped_path(mode, mid)
            assert path == _expected_path(mode, mid)
            reached.add(("register", mid // 256, mode) if path == 0 else ("general", path, mode))
    assert {r[:2] for r in reached if r[0] == "register"} == {("register", it) for it in (1, 2, 3, 4)}
    assert {r[1:] for r in reached if r[0] == "general"} == {(pw, mode) for pw in (4, 2, 1) for mode in (0, 1, 2)}
    assert {r[2] for r in reached if r[0] == "register"} == {0, 1}


@pytest.mark.parametrize("kind", ["empty", "single", "shuffled"])
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("N,B,P,mid,G", SCORE_SHAPES)
def test_attr_score_grouped_matches_float64(N, B, P, mid, G, mode, kind):
    ops = _ops()
    g = torch.Generator().manual_seed(N * 1000 + B * 10 + mode)
    vp = torch.randn(N * P, mid, generator=g)
    qp = torch.randn(B, mid, generator=g)
    wx = torch.randn(G, 2 * mid if mode == 2 else mid, generator=g)
    ds = torch.randn(B, G, P, generator=g)
    r1 = torch.randn(B, P, generator=g)
    img = _grouping(kind, N, B, g)
    order, offsets = group_by_image(img, N)
    want = R.score_half(r1, ds, vp.view(N, P, mid), qp, wx, img, mode)
    d = lambda t: t.to(DEV)
    tag = f"{N,B,P,mid,G} mode {mode} {kind} path {ops.att_attr_score_grouped_path(mode, mid)}"
    out = torch.full((B, P), 7.0, device=DEV)
    ops.att_attr_score_grouped(d(r1), d(ds), d(vp), d(qp), d(wx), d(order), d(offsets), N, B, P, mode, out=out)
    torch.cuda.synchronize()
    check(f"att_attr_score_grouped {tag}", out, want, 3e-6)                              # every element
    # '|' reads no q'
    if mode == 2:
        out_noq = ops.att_attr_score_grouped(d(r1), d(ds), d(vp), None, d(wx), d(order), d(offsets), N, B, P, mode)
        assert torch.equal(out_noq, out)
    # questions that are not listed keep what the output held: un-list the questions of the first image that has some
    first = int(img.min())
    cut = offsets.clone()
    cut[:first + 1] = offsets[first + 1]
    kept = torch.full((B, P), 7.0, device=DEV)
    ops.att_attr_score_grouped(d(r1), d(ds), d(vp), d(qp), d(wx), d(order), d(cut), N, B, P, mode, out=kept)
    torch.cuda.synchronize()
    unlisted = d(img == first)
    assert bool(unlisted.any()) and bool((kept[unlisted] == 7.0).all()) and torch.equal(kept[~unlisted], out[~unlisted])
    # the pairs form over a table of distinct questions: the plain form on qp[qrow], bit for bit
    M = 3
    table = torch.randn(M, mid, generator=g)
    qrow = torch.randint(0, M, (B,), generator=g)
    out_p = ops.att_attr_score_grouped(d(r1), d(ds), d(vp), d(table), d(wx), d(order), d(offsets), N, B, P, mode,
                                       qrow=d(qrow.to(torch.int32)))
    out_e = ops.att_attr_score_grouped(d(r1), d(ds), d(vp), d(table[qrow]), d(wx), d(order), d(offsets), N, B, P, mode)
    # a float16 v': the fp32 form on the widened values, bit for bit (both forms)
    vh = d(vp).half()
    out_h = ops.att_attr_score_grouped(d(r1), d(ds), vh, d(qp), d(wx), d(order), d(offsets), N, B, P, mode)
    out_w = ops.att_attr_score_grouped(d(r1), d(ds), vh.float(), d(qp), d(wx), d(order), d(offsets), N, B, P, mode)
    out_hp = ops.att_attr_score_grouped(d(r1), d(ds), vh, d(table), d(wx), d(order), d(offsets), N, B, P, mode,
                                        qrow=d(qrow.to(torch.int32)))
    out_wp = ops.att_attr_score_grouped(d(r1), d(ds), vh.float(), d(table[qrow]), d(wx), d(order), d(offsets), N, B, P, mode)
    torch.cuda.synchronize()
    assert torch.equal(out_p, out_e)
    assert torch.equal(out_h, out_w) and torch.equal(out_hp, out_wp)


# ----------------------------------------------------------------------------- the whole path on the golden fixtures
def _parity(tag, att, do_option, bound=2e-4):
    ref, r1, r2 = R.fixture_reference(do_option, att.answers.tolist())
    B = ref.shape[0]
    e = rel(att.maps.reshape(B, -1), ref)
    print(f"[parity-explain] {tag}: maps max|err|/max|ref| = {e:.3e} (bound {bound:.0e}), max|R| {float(ref.abs().max()):.3e}, "
          f"max|r1| {float(r1.abs().max()):.3e}, max|r2| {float(r2.abs().max()):.3e}")
    assert e < bound
    return e


@pytest.mark.parametrize("do_option", ["+", "*", "|"])
def test_explain_matches_autograd_on_fixtures(do_option):
    f, m, feats = _fixture_model(do_option)
    name = R.FIXTURES[do_option]
    q, ql, img = f["q"].to(DEV), f["q_len"].to(DEV), list(R.IMAGE_INDEX)
    B, A = len(img), f["cfg"]["max_answers"]
    att = m.explain(feats, q, ql, img)
    torch.cuda.synchronize()
    assert isinstance(att, Attribution) and att.maps.shape == (B, *feats.grid) and att.maps.dtype == torch.float32
    assert att.answers.dtype == torch.int64 and att.answers.shape == (B,) and att.logits.shape == (B, A)
    assert not att.maps.requires_grad and m._last_ctx is None
    # logits are answer()'s, answers are predict()'s arg-max
    assert torch.equal(att.logits, m.answer(feats, q, ql, img))
    assert torch.equal(att.answers, m.predict(feats, q, ql, img, k=1).indices[:, 0])
    _parity(f"{name} explain arg-max", att, do_option)
    # given columns: a list, a CUDA tensor (taken as it is), an out-of-range CUDA entry (a map of zeros)
    cols = [(3 * b + 1) % A for b in range(B)]
    given = m.explain(feats, q, ql, img, answers=cols)
    assert given.answers.tolist() == cols and torch.equal(given.logits, att.logits)
    _parity(f"{name} explain given columns", given, do_option)
    on_dev = m.explain(feats, q, ql, img, answers=torch.tensor(cols, device=DEV))
    assert torch.equal(on_dev.maps, given.maps) and torch.equal(on_dev.answers, given.answers)
    bad = torch.tensor(cols, device=DEV)
    bad[2] = A
    zero = m.explain(feats, q, ql, img, answers=bad)
    assert float(zero.maps[2].abs().max()) == 0.0 and torch.equal(zero.maps[:2], given.maps[:2])
    assert torch.equal(zero.maps[3:], given.maps[3:])
    # the same pairs from the two caches
    qu, qlu, qidx = unique_questions(f["q"], f["q_len"])
    assert qu.shape[0] < B
    qfeats = m.encode_questions(qu.to(DEV), qlu.to(DEV))
    pairs = m.explain_pairs(feats, qfeats, img, qidx)
    assert torch.equal(pairs.logits, m.answer_pairs(feats, qfeats, img, qidx))
    assert torch.equal(pairs.answers, m.predict_pairs(feats, qfeats, img, qidx, k=1).indices[:, 0])
    _parity(f"{name} explain_pairs arg-max", pairs, do_option)
    pairs_given = m.explain_pairs(feats, qfeats, img, qidx, answers=cols)
    _parity(f"{name} explain_pairs given columns", pairs_given, do_option)
    # an empty batch
    none = m.explain(feats, q[:0], ql[:0], [])
    assert none.maps.shape == (0, *feats.grid) and none.answers.shape == (0,) and none.logits.shape == (0, A)
    none = m.explain_pairs(feats, qfeats, [], [])
    assert none.maps.shape == (0, *feats.grid) and none.answers.dtype == torch.int64
    assert m._last_ctx is None and all(p.grad is None for p in m.parameters())


def test_explain_fp32x3_and_a_float16_cache():
    f, m, feats = _fixture_model("+", "fp32x3")
    q, ql, img = f["q"].to(DEV), f["q_len"].to(DEV), list(R.IMAGE_INDEX)
    att = m.explain(feats, q, ql, img)
    assert torch.equal(att.logits, m.answer(feats, q, ql, img))
    _parity("tiny_plus explain fp32x3", att, "+")
    # a float16 cache gives what its widened copy gives, bit for bit, through both calls
    for do_option in ("*", "|"):
        f, m, feats = _fixture_model(do_option)
        q, ql = f["q"].to(DEV), f["q_len"].to(DEV)
        f16 = feats.to(torch.float16)
        f32 = f16.to(torch.float32)
        a16, a32 = m.explain(f16, q, ql, img), m.explain(f32, q, ql, img)
        assert torch.equal(a16.maps, a32.maps) and torch.equal(a16.logits, a32.logits) and torch.equal(a16.answers, a32.answers)
        qu, qlu, qidx = unique_questions(f["q"], f["q_len"])
        qfeats = m.encode_questions(qu.to(DEV), qlu.to(DEV))
        p16, p32 = m.explain_pairs(f16, qfeats, img, qidx), m.explain_pairs(f32, qfeats, img, qidx)
        assert torch.equal(p16.maps, p32.maps) and torch.equal(p16.logits, p32.logits)
        # against the unrounded features: one rounding of vn and v' to 11 significand bits
        full = m.explain(feats, q, ql, img, answers=a16.answers)
        e = rel(a16.maps, full.maps)
        print(f"[parity-explain] {R.FIXTURES[do_option]} float16 cache vs fp32 cache: maps max|diff|/max = {e:.3e}")


# ----------------------------------------------------------------------------- order invariance, bit for bit
def _assert_order_and_split_invariant(m, feats, q, ql, image_index, seed):
    B = q.shape[0]
    a0 = m.explain(feats, q.to(DEV), ql.to(DEV), image_index)
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(seed))
    # the same columns explained: a permuted batch must not depend on a re-run arg-max either, but pin them all the same
    a1 = m.explain(feats, q[perm].to(DEV), ql[perm].to(DEV), image_index[perm])
    torch.cuda.synchronize()
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(B)
    assert torch.equal(a1.maps[inv.to(DEV)], a0.maps)
    assert torch.equal(a1.answers[inv.to(DEV)], a0.answers) and torch.equal(a1.logits[inv.to(DEV)], a0.logits)
    h = B // 3
    lo = m.explain(feats, q[:h].to(DEV), ql[:h].to(DEV), image_index[:h])
    hi = m.explain(feats, q[h:].to(DEV), ql[h:].to(DEV), image_index[h:])
    assert torch.equal(torch.cat([lo.maps, hi.maps]), a0.maps)
    assert torch.equal(torch.cat([lo.answers, hi.answers]), a0.answers)


def test_order_and_split_invariance_register_kernel():
    from oracle import vqa_oracle as O
    V, N, B, T = 200, 5, 24, 8
    torch.manual_seed(9)
    m = build(full_cfg(50), V).eval()                              # mid = 1024, '+': the register kernel
    v, q, _, _, _, _, ql = O.synthetic_batch(B, 64, T, V, 50, seed=11)
    feats = m.encode_images(v[:N].to(DEV))
    image_index = torch.randint(0, N, (B,), generator=torch.Generator().manual_seed(12))
    _assert_order_and_split_invariant(m, feats, q, ql, image_index, seed=13)


@pytest.mark.parametrize("do_option", ["*", "|"])
def test_order_and_split_invariance_general_kernel(do_option):
    f, m, feats = _fixture_model(do_option)                         # mid = 24: the general kernel
    _assert_order_and_split_invariant(m, feats, f["q"], f["q_len"], f["img"], seed=3)


# ----------------------------------------------------------------------------- against the path that exists today
def test_logits_match_forward_and_forward_backward_are_unchanged_after_explain():
    from dl_vqa_amd.train import soft_ce_loss_and_score
    g = Golden("tiny_plus")
    cfg = tiny_cfg(g.meta)
    v, q, ql = g.t["v"].to(DEV), g.t["q"].to(DEV), g.t["q_len"].to(DEV)
    a_idx, a_val = g.t["a_idx"].to(DEV), g.t["a_val"].to(DEV)

    def step(m):
        y = m(v, q, ql)
        soft_ce_loss_and_score(y, a_idx, a_val)[0].backward()
        torch.cuda.synchronize()
        return y.detach().clone(), {k: p.grad.clone() for k, p in m.named_parameters()}

    fresh = build(cfg, g.meta["V"], g.sd).eval()
    y_f, g_f = step(fresh)

    m = build(cfg, g.meta["V"], g.sd).eval()
    m._ensure_flat()
    flat_grad = m._flat_grad
    flat_grad.fill_(3.0)
    torch.manual_seed(77)
    rng = torch.get_rng_state()
    feats = m.encode_images(v)
    idx = list(range(q.shape[0]))
    att = m.explain(feats, q, ql, idx)
    qfeats = m.encode_questions(q, ql)
    m.explain_pairs(feats, qfeats, idx, idx, answers=att.answers)
    torch.cuda.synchronize()
    # forward(v[idx]) is the only route to an explanation today; it cannot give d / d vn, so the logits are compared
    assert float((att.logits - y_f).abs().max()) < 1e-5
    assert m._last_ctx is None and len(m._pending) == 0
    assert m._flat_grad is flat_grad and bool((flat_grad == 3.0).all())
    assert torch.equal(torch.get_rng_state(), rng)                  # the dropout seed stream was not drawn from
    assert all(p.grad is None for p in m.parameters())
    flat_grad.zero_()
    y_m, g_m = step(m)
    assert torch.equal(y_m, y_f)
    for k in g_f:
        assert torch.equal(g_m[k], g_f[k]), k
    # refusals that need a device: foreign features, a bank without v', train mode
    with pytest.raises(RuntimeError, match="belong elsewhere"):
        fresh.explain(feats, q, ql, idx)
    with pytest.raises(RuntimeError, match="with_vprime=False"):
        m.explain(m.encode_images(v, with_vprime=False), q, ql, idx)
    with pytest.raises(IndexError):
        m.explain(feats, q, ql, idx[:-1] + [feats.N])
    m.train()
    with pytest.raises(RuntimeError, match="training mode"):
        m.explain(feats, q, ql, idx)
