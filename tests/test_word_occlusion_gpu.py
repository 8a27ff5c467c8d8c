"""GPU: exact word occlusion from cached features -- vqa_lstm_occl_cell_fwd and vqa_occl_words against float64
(tests/word_occlusion_ref.py) on synthetic inputs, VqaNet.explain_words_occlusion on the golden fixtures and on random models
whose base run takes the fused recurrence, against the float64 brute force and against the brute-force route through the
public API (answer() on the questions with the padding token substituted), chunking, cache types, batch invariance, and the
existing paths untouched.

The whole-path bound is measured on code that is not under test, as tests/test_occlusion_gpu._bound does: the largest absolute
difference, over the three fixtures and both column choices, between the public brute-force route and float64, times 4 (the
new route adds a second recurrence schedule and a dot-product tail to the same products), and not below 1e-7 (one ulp of a 0.27
logit is 3e-8; a faithful fp32 CPU evaluation is 2.3e-8 from float64 on these fixtures).  max|words| is 0.011 .. 0.047 on the
fixtures and the gradient x input words are 63 % .. 125 % of that away (tests/test_word_occlusion_cpu.py), so zeros or the
first-order values are 5 orders of magnitude outside it."""
import functools

import pytest
import torch

from dl_vqa_amd import WordOcclusion
from dl_vqa_amd.model import word_occlusion_chunks, word_occlusion_table
from tests import attribution_ref as R
from tests import word_attribution_ref as W
from tests import word_occlusion_ref as WO
from tests.explain_util import build, off_by_one_float as _off_by_one_float, within
from tests.golden_util import Golden, tiny_cfg
from tests.test_kernels_gpu import check

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_within = functools.partial(within, label="parity-word-occlusion")
MODELS = [("+", "fp32"), ("*", "fp32"), ("|", "fp32"), ("+", "fp32x3")]


def _ops():
    from dl_vqa_amd import ops
    return ops


d = lambda t: None if t is None else t.to(DEV)


def _lengths(B, T, g):
    q_len = torch.randint(1, T + 1, (B,), generator=g)
    q_len[0], q_len[-1] = T, 1                                      # ragged, T and 1 included (B >= 2)
    return q_len


# ----------------------------------------------------------------------------- kernel 1: the variant cell
@pytest.mark.parametrize("n,B,T,H", [(7, 3, 5, 16), (1, 2, 1, 32), (9, 5, 7, 20), (6, 4, 14, 36), (5, 3, 4, 6)])
def test_variant_cell_matches_the_float64_step(n, B, T, H):
    """Every s in [0, T): below, at and above a row's t, and at and above q_len[b].  H = 6 takes the scalar form."""
    ops = _ops()
    g = torch.Generator().manual_seed(1000 * n + 100 * B + 10 * T + H)
    ld, cf_ld = H + 4, 2 * H + 4                                    # row strides wider than H
    xg_base, xg0 = torch.randn(T, B, 4 * H, generator=g), torch.randn(4 * H, generator=g)
    hg = torch.randn(n, 4 * H, generator=g)
    h0, c0 = torch.tanh(torch.randn(n, H, generator=g)), torch.randn(n, H, generator=g)
    q_len = _lengths(B, T, g)
    var_b = torch.randint(0, B, (n,), generator=g).to(torch.int32)
    var_t = torch.stack([torch.randint(0, int(q_len[b]), (1,), generator=g)[0] for b in var_b.tolist()]).to(torch.int32)
    # the longest question's first and last slot (s at and above t, resp. below it) and the shortest question (held from s = 1 on)
    for r, (b, t) in enumerate([(0, 0), (B - 1, 0), (0, T - 1)][:n]):
        var_b[r], var_t[r] = b, t
    cf_row = torch.randperm(n, generator=g).to(torch.int32)

    def run(s, xg=None, rows=n, final=True):
        hb, cb = torch.full((n, ld), 7.0, device=DEV), torch.full((n, ld), 7.0, device=DEV)
        hb[:, :H], cb[:, :H] = d(h0), d(c0)
        cf = torch.full((n, cf_ld), 7.0, device=DEV)
        ops.lstm_occl_cell_fwd(d(xg_base) if xg is None else xg, d(xg0), d(hg), hb[:, :H], cb[:, :H], d(q_len), d(var_b), d(var_t),
                               s, rows, c_final=cf[:, H:] if final else None, cf_row=d(cf_row) if final else None)
        torch.cuda.synchronize()
        return hb, cb, cf

    seen = set()
    for s in range(T):
        hb, cb, cf = run(s)
        want_h, want_c = WO.cell_step(xg_base, xg0, hg, h0, c0, q_len, var_b, var_t, s)
        tag = f"lstm_occl_cell {n,B,T,H} s={s}"
        check(f"{tag} h", hb[:, :H], want_h, 3e-6)
        check(f"{tag} c", cb[:, :H], want_c, 3e-6)
        held = q_len[var_b.long()] <= s
        at = (var_t == s) & ~held
        seen |= {"held"} if bool(held.any()) else set()
        seen |= {"at"} if bool(at.any()) else set()
        seen |= {"below"} if bool(((var_t > s) & ~held).any()) else set()
        seen |= {"above"} if bool(((var_t < s) & ~held).any()) else set()
        # held rows are bit-unchanged and write no c_final; the padding between H and the row stride is never touched
        assert torch.equal(hb[d(held), :H], d(h0)[d(held)]) and torch.equal(cb[d(held), :H], d(c0)[d(held)])
        assert bool((hb[:, H:] == 7.0).all()) and bool((cb[:, H:] == 7.0).all())
        assert bool((cf[:, :H] == 7.0).all()) and bool((cf[:, 2 * H:] == 7.0).all())
        rows = d(cf_row.long())
        assert torch.equal(cf[rows][d(~held), H:2 * H], cb[d(~held), :H]) and bool((cf[rows][d(held), H:2 * H] == 7.0).all())
        # rows at s == t read xg0, not the base row: with the base row they would be somewhere else
        if bool(at.any()):
            other_h, _ = WO.cell_step(xg_base, xg0, hg, h0, c0, q_len, var_b, torch.full_like(var_t, -1), s)
            assert float((other_h - want_h)[at].abs().max()) > 1e-3
        # a misaligned xg_base (the scalar form) gives the aligned call's bits; no c_final gives the same states
        h2, c2, _ = run(s, xg=_off_by_one_float(d(xg_base)))
        assert torch.equal(h2, hb) and torch.equal(c2, cb)
        h3, c3, cf3 = run(s, final=False)
        assert torch.equal(h3, hb) and torch.equal(c3, cb) and bool((cf3 == 7.0).all())
    assert {"at"} <= seen and (T == 1 or {"held", "above"} <= seen)
    # the first `rows` rows only; n == 0 launches nothing
    if n > 1:
        hb, cb, _ = run(0)
        hp, cp, _ = run(0, rows=n - 1)
        assert torch.equal(hp[:n - 1], hb[:n - 1]) and torch.equal(hp[n - 1, :H], d(h0)[n - 1]) and torch.equal(cp[n - 1, :H], d(c0)[n - 1])
    hz, cz, cfz = run(0, rows=0)
    assert torch.equal(hz[:, :H], d(h0)) and torch.equal(cz[:, :H], d(c0)) and bool((cfz == 7.0).all())


# ----------------------------------------------------------------------------- kernel 2: the tail
@pytest.mark.parametrize("B,T,hid,A", [(3, 5, 24, 11), (2, 1, 1024, 7), (4, 14, 36, 3000), (3, 4, 6, 5)])
def test_tail_matches_float64(B, T, hid, A):
    ops = _ops()
    g = torch.Generator().manual_seed(1000 * B + 100 * T + hid + A)
    q_len = _lengths(B, T, g)
    tab = word_occlusion_table(q_len, T)
    n = tab.V
    h1 = torch.relu(torch.randn(n, hid, generator=g))
    W2, b2 = torch.randn(A, hid, generator=g), torch.randn(A, generator=g)
    logits = torch.randn(B, A, generator=g)
    answers = torch.randint(0, A, (B,), generator=g).to(torch.int32)
    answers[0] = A                                                  # an out-of-range column on the longest question
    want = WO.tail(h1, W2, b2, answers, logits, tab.fwd_b, tab.fwd_t, q_len, B, T)
    args = (d(W2), d(b2), d(answers), d(logits), d(tab.fwd_b), d(tab.fwd_t), d(q_len))
    out = torch.full((B, T), 7.0, device=DEV)
    ops.occl_words(d(h1), *args, out)
    torch.cuda.synchronize()
    check(f"occl_words {B,T,hid,A}", out, want, 3e-6)
    assert bool((out != 7.0).all())                                 # every element is written
    pad = d(torch.arange(T)[None, :] >= q_len[:, None])
    zero = out[pad | (torch.arange(B, device=DEV) == 0)[:, None]]
    assert bool((zero == 0.0).all()) and not bool(torch.signbit(zero).any())
    assert float(out[1:].abs().max()) > 0
    # the scalar form on the same values (a misaligned h1, then a misaligned W2): the same bits.  hid % 4 != 0 is scalar already
    for which in (0, 1):
        again = torch.full((B, T), 7.0, device=DEV)
        ops.occl_words(_off_by_one_float(d(h1)) if which == 0 else d(h1), _off_by_one_float(d(W2)) if which == 1 else d(W2),
                       *args[1:], again)
        torch.cuda.synchronize()
        assert torch.equal(again, out), which
    # question by question: each call writes every element of its rows and nothing else
    parts = torch.full((B, T), 7.0, device=DEV)
    for b in range(B):
        sub = word_occlusion_table(q_len, T, b, b + 1)
        rows = [r for r, vb in enumerate(tab.fwd_b.tolist()) if vb == b]
        assert tab.fwd_t[rows].tolist() == sub.fwd_t.tolist()
        ops.occl_words(d(h1)[rows], *args[:4], d(sub.fwd_b), d(sub.fwd_t), args[6], parts, b, 1)
        torch.cuda.synchronize()
        assert torch.equal(parts[:b + 1], out[:b + 1]) and bool((parts[b + 1:] == 7.0).all())
    # no variant rows: the zeros of the rows are still written
    empty = torch.full((B, T), 7.0, device=DEV)
    none = torch.zeros(0, dtype=torch.int32, device=DEV)
    ops.occl_words(torch.zeros(0, hid, device=DEV), *args[:4], none, none, torch.zeros(B, dtype=torch.int64, device=DEV), empty)
    torch.cuda.synchronize()
    assert bool((empty == 0.0).all())


def test_xg0_is_the_base_products_row_for_a_zero_input():
    """b_ih + b_hh as the question encoder's xg product writes it for an all-zero input row, at the batch's size and at one row."""
    ops = _ops()
    g = Golden("tiny_plus")
    m = build(tiny_cfg(g.meta), g.meta["V"], g.sd).eval()
    m._ensure_flat()
    P, eng = m._param_dict(), m._engine
    w, b1, b2 = P["text.lstm.weight_ih_l0"], P["text.lstm.bias_ih_l0"], P["text.lstm.bias_hh_l0"]
    rows = {}
    for M in (1, 35, 256 * 14):
        out = torch.empty(M, 4 * eng.H, device=DEV)
        ops.gemm(torch.zeros(M, eng.E, device=DEV), w, out, M, 4 * eng.H, eng.E, bias1=b1, bias2=b2, tag=10)
        torch.cuda.synchronize()
        assert bool((out == out[:1]).all())
        rows[M] = out[0].clone()
    assert torch.equal(rows[1], rows[35]) and torch.equal(rows[1], rows[256 * 14])
    check("xg0 vs b_ih + b_hh", rows[1], b1.double() + b2.double(), 1e-6)


# ----------------------------------------------------------------------------- the whole path
def _model(case, compute_dtype="fp32"):
    V = case["V"] if "V" in case else case["golden"].meta["V"]
    m = build(case["cfg"], V, WO.case_sd(case), compute_dtype).eval()
    return m, m.encode_images(case["v"].to(DEV))


def _substituted(q, q_len):
    """Every variant (b, t), b-major, as a question of its own with the padding token at slot t."""
    pairs = WO.variants(q_len, q.shape[1])
    vb = torch.tensor([b for b, _ in pairs])
    qs = q[vb].clone()
    qs[torch.arange(len(pairs)), torch.tensor([t for _, t in pairs])] = 0
    return pairs, vb, qs


@functools.lru_cache(maxsize=None)
def _fixture_run(do_option, compute_dtype):
    """The model of a fixture, its features, answer() on the questions and on every substituted question: the brute-force
    route through the public API, valid while row 0 of the embedding is zero."""
    f = R.fixture_case(do_option)
    m, feats = _model(f, compute_dtype)
    assert float(m.text.embedding.weight[0].detach().abs().max()) == 0.0
    q, ql, img = f["q"], f["q_len"], torch.tensor(R.IMAGE_INDEX)
    pairs, vb, qs = _substituted(q, ql)
    full = m.answer(feats, q.to(DEV), ql.to(DEV), img)
    occluded = m.answer(feats, qs.to(DEV), ql[vb].to(DEV), img[vb])
    torch.cuda.synchronize()
    return dict(f=f, m=m, feats=feats, q=q.to(DEV), ql=ql.to(DEV), img=img.tolist(), full=full, occluded=occluded, pairs=pairs)


def _route_words(run, cols):
    """words [B, T] of the public brute-force route: the base logit minus the substituted question's, at each question's column."""
    B, T = run["q"].shape
    words = torch.zeros(B, T, dtype=torch.float64)
    full, occluded = run["full"].double().cpu(), run["occluded"].double().cpu()
    for r, (b, t) in enumerate(run["pairs"]):
        words[b, t] = full[b, cols[b]] - occluded[r, cols[b]]
    return words


def _column_choices(run):
    B, A = run["full"].shape
    return run["full"].argmax(1).tolist(), WO.columns(B, A)


@functools.lru_cache(maxsize=None)
def _bound(compute_dtype):
    worst = 0.0
    for do_option in ("+", "*", "|"):
        run = _fixture_run(do_option, compute_dtype)
        for cols in _column_choices(run):
            worst = max(worst, float((_route_words(run, cols) - WO.fixture_brute(do_option, cols)).abs().max()))
    bound = max(4 * worst, 1e-7)
    print(f"[parity-word-occlusion] {compute_dtype}: answer() on the substituted questions vs float64 brute force, max|diff| over "
          f"the three fixtures = {worst:.3e}; whole-path bound = max(4 x that, 1e-7) = {bound:.3e}")
    return bound


@pytest.mark.parametrize("do_option,compute_dtype", MODELS)
def test_words_match_float64_and_the_brute_force_route(do_option, compute_dtype):
    run = _fixture_run(do_option, compute_dtype)
    bound = _bound(compute_dtype)
    m, feats, q, ql, img = run["m"], run["feats"], run["q"], run["ql"], run["img"]
    name = f"{R.FIXTURES[do_option]} {compute_dtype}"
    B, T = q.shape
    A = run["full"].shape[1]
    top, given = _column_choices(run)
    pad = (torch.arange(T, device=DEV)[None, :] >= ql[:, None])
    assert bool(pad.any())
    for what, cols, arg in (("arg-max", top, None), ("given columns", given, given)):
        got = m.explain_words_occlusion(feats, q, ql, img, answers=arg)
        torch.cuda.synchronize()
        assert isinstance(got, WordOcclusion) and got.words.shape == (B, T) and got.words.dtype == torch.float32
        assert got.answers.dtype == torch.int64 and got.answers.tolist() == cols and not got.words.requires_grad
        assert m._last_ctx is None
        att = m.explain(feats, q, ql, img, answers=arg)                 # answers and logits: explain's bits
        assert torch.equal(got.answers, att.answers) and torch.equal(got.logits, att.logits) and torch.equal(got.logits, run["full"])
        assert bool((got.words[pad] == 0.0).all()) and not bool(torch.signbit(got.words[pad]).any())
        ref = WO.fixture_brute(do_option, cols)
        assert float(ref.abs().max()) > 1e-2
        _within(f"{name} {what} vs float64", got.words, ref, bound)
        _within(f"{name} {what} vs the brute-force route", got.words, _route_words(run, cols), bound)
    # an out-of-range CUDA column: a row of zeros, the other rows as they were
    bad = torch.tensor(given, device=DEV)
    bad[2] = A
    zero = m.explain_words_occlusion(feats, q, ql, img, answers=bad)
    assert float(zero.words[2].abs().max()) == 0.0 and torch.equal(zero.words[:2], got.words[:2])
    assert torch.equal(zero.words[3:], got.words[3:])
    # a slot whose embedding row is zero already (token 0 inside a question, an id outside the vocabulary): not forced to
    # zero -- the difference of two routes to the same value, within the bound
    q0 = q.clone()
    q0[0, 1] = 0
    z = m.explain_words_occlusion(feats, q0, ql, img, answers=given)
    assert int(ql[0]) > 1 and abs(float(z.words[0, 1])) <= bound
    _within(f"{name} the other questions beside a zero-row slot", z.words[1:], got.words[1:], bound)


@pytest.mark.parametrize("bidirectional", [True, False])
def test_on_the_fused_base_recurrence(bidirectional):
    """The fixtures have H = 16 (the base run steps per launch pair); these models have H = 32 and take vqa_lstm_seq_fwd."""
    bound = _bound("fp32")
    for T in (6, 1):
        case = W.random_case(bidirectional, T)
        m, feats = _model(case)
        assert m._engine._lstm_schedule()[0] and m._engine.ndir == (2 if bidirectional else 1)
        q, ql, img = case["q"].to(DEV), case["q_len"].to(DEV), case["img"]
        B, A = q.shape[0], case["cfg"]["max_answers"]
        got = m.explain_words_occlusion(feats, q, ql, img)
        torch.cuda.synchronize()
        pad = (torch.arange(T, device=DEV)[None, :] >= ql[:, None])
        assert bool((got.words[pad] == 0.0).all())
        tag = f"random H=32 {'bi' if bidirectional else 'uni'}directional T={T}"
        _within(f"{tag} arg-max vs float64", got.words, WO.case_brute(case, "+", got.answers.tolist()), bound)
        cols = WO.columns(B, A)
        given = m.explain_words_occlusion(feats, q, ql, img, answers=cols)
        _within(f"{tag} given columns vs float64", given.words, WO.case_brute(case, "+", cols), bound)


def test_chunks_a_float16_cache_and_batch_invariance():
    bound = _bound("fp32")
    run = _fixture_run("+", "fp32")
    m, feats, q, ql, img = run["m"], run["feats"], run["q"], run["ql"], run["img"]
    B, T = q.shape
    whole = m.explain_words_occlusion(feats, q, ql, img)
    # several chunks: within the bound of one chunk (bit equality is not claimed: the GEMM plans may depend on the row count)
    lengths = ql.tolist()
    for cap in (6, 1):
        n_chunks = len(word_occlusion_chunks(lengths, T, cap))
        assert n_chunks >= 3
        cut = m.explain_words_occlusion(feats, q, ql, img, _variant_rows=cap)
        assert torch.equal(cut.logits, whole.logits) and torch.equal(cut.answers, whole.answers)
        _within(f"tiny_plus {n_chunks} chunks (at most {cap} variants each) vs one chunk", cut.words, whole.words, bound)
    # cap 1: every question is alone in its chunk -- its row is what the question gives when asked alone
    assert len(word_occlusion_chunks(lengths, T, 1)) == B
    for b in (0, 2, B - 1):
        alone = m.explain_words_occlusion(feats, q[b:b + 1], ql[b:b + 1], img[b:b + 1], answers=whole.answers[b:b + 1])
        _within(f"tiny_plus question {b} alone in its chunk vs asked alone", cut.words[b], alone.words[0], bound)
    for do_option in ("+", "*", "|"):
        run = _fixture_run(do_option, "fp32")
        m, feats, q, ql = run["m"], run["feats"], run["q"], run["ql"]
        # a float16 cache gives what its widened copy gives, bit for bit
        f16 = feats.to(torch.float16)
        a16, a32 = m.explain_words_occlusion(f16, q, ql, img), m.explain_words_occlusion(f16.to(torch.float32), q, ql, img)
        assert torch.equal(a16.words, a32.words) and torch.equal(a16.logits, a32.logits) and torch.equal(a16.answers, a32.answers)
        assert float(a16.words.abs().max()) > 1e-3
        # a split and permuted batch: within the bound of the whole
        a0 = m.explain_words_occlusion(feats, q, ql, img)
        perm = torch.randperm(B, generator=torch.Generator().manual_seed(3))
        idx = torch.tensor(img)
        h = B // 3
        lo = m.explain_words_occlusion(feats, q[perm[:h]], ql[perm[:h]], idx[perm[:h]], answers=a0.answers[perm[:h].to(DEV)])
        hi = m.explain_words_occlusion(feats, q[perm[h:]], ql[perm[h:]], idx[perm[h:]], answers=a0.answers[perm[h:].to(DEV)])
        _within(f"{R.FIXTURES[do_option]} split and permuted batch vs whole", torch.cat([lo.words, hi.words]),
                a0.words[perm.to(DEV)], bound)
    # an empty batch
    none = m.explain_words_occlusion(feats, q[:0], ql[:0], [])
    assert none.words.shape == (0, T) and none.answers.shape == (0,) and none.logits.shape == (0, run["full"].shape[1])
    assert none.answers.dtype == torch.int64 and m._last_ctx is None


def test_forward_and_backward_are_unchanged_after_explain_words_occlusion():
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
    y0, g0 = step(fresh)

    m = build(cfg, g.meta["V"], g.sd).eval()
    m._ensure_flat()
    flat_grad = m._flat_grad
    flat_grad.fill_(3.0)
    torch.manual_seed(77)
    rng = torch.get_rng_state()
    feats = m.encode_images(v)
    idx = list(range(q.shape[0]))
    got = m.explain_words_occlusion(feats, q, ql, idx, _variant_rows=4)
    torch.cuda.synchronize()
    assert torch.equal(got.logits, m.answer(feats, q, ql, idx)) and float(got.words.abs().max()) > 1e-3
    assert m._last_ctx is None and len(m._pending) == 0
    assert m._flat_grad is flat_grad and bool((flat_grad == 3.0).all())
    assert torch.equal(torch.get_rng_state(), rng)                  # the dropout seed stream was not drawn from
    assert all(p.grad is None for p in m.parameters())
    flat_grad.zero_()
    y1, g1 = step(m)
    assert torch.equal(y1, y0)
    for k in g0:
        assert torch.equal(g1[k], g0[k]), k
    # refusals that need a device: foreign features, an index outside the cache
    with pytest.raises(RuntimeError, match="belong elsewhere"):
        fresh.explain_words_occlusion(feats, q, ql, idx)
    with pytest.raises(IndexError):
        m.explain_words_occlusion(feats, q, ql, idx[:-1] + [feats.N])
