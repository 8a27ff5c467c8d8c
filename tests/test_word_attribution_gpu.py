"""GPU: per-token gradient x input -- vqa_att_attr_dq_grouped and vqa_embed_attr against float64 and against the code they
share (tests/word_attribution_ref.py), VqaNet.explain_words on the golden fixtures and on random models that take the fused
recurrence, stage by stage against autograd through the oracle, and the existing paths untouched.

The attention path carries 4e-4 ('+') and 4e-5 ('*') of max|words| on the fixtures: a bound on `words` alone would pass with
kernel A returning zeros, so its stage (stages["dq_att"]) is checked against the attention-only reference relative to ITS
maximum.  Bounds: dq_att 2e-4 (what test_attribution_gpu._parity applies to maps, the same probs -> dscore -> walk chain);
words 2e-5 (tests/test_lstm_gpu.py's bound for dgates, of which words is a linear image through W_ih and the embedding row),
times sqrt(T / 5) for T > 5 as there."""
import math

import pytest
import torch

from dl_vqa_amd import WordAttribution, group_by_image
from tests import attribution_ref as R
from tests import word_attribution_ref as W
from tests.explain_util import build, grouping as _grouping, off_by_one_float as _off_by_one_float, rel
from tests.golden_util import Golden, tiny_cfg
from tests.test_kernels_gpu import check

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DQ_BOUND, WORDS_BOUND = 2e-4, 2e-5


def _ops():
    from dl_vqa_amd import ops
    return ops


# ----------------------------------------------------------------------------- kernel A: d logit / d q' through the scores
# tests/test_shared_train_gpu.py::SHAPES with 676 and 169 positions cut to 33 and 18, then mid = 768 and 512 (the register
# kernel's IT = 3 and 2 beside 1 and 4) and mid = 2304: the general kernel walks 4, 2 and 1 quads per thread at 520, 2048 / 24
# and 2304; P below, at and above a 16-position tile with a ragged last tile; G = 1..4
DQ_SHAPES = [(3, 7, 4, 24, 2), (2, 9, 33, 1024, 2), (5, 5, 18, 256, 1), (3, 6, 20, 520, 4), (2, 5, 37, 2048, 3),
             (2, 4, 9, 768, 3), (2, 3, 5, 512, 1), (2, 4, 6, 2304, 2)]


@pytest.mark.parametrize("kind", ["empty", "single", "shuffled"])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("N,B,P,mid,G", DQ_SHAPES)
def test_attr_dq_grouped_matches_float64_and_the_training_kernel(N, B, P, mid, G, mode, kind):
    from dl_vqa_amd._lib import VqaHipError
    ops = _ops()
    g = torch.Generator().manual_seed(N * 1000 + B * 10 + mode)
    vp = torch.randn(N * P, mid, generator=g)
    qp = torch.randn(B, mid, generator=g)
    wx = torch.randn(G, mid, generator=g)
    ds = torch.randn(B, G, P, generator=g)
    img = _grouping(kind, N, B, g)
    order, offsets = group_by_image(img, N)
    # float64 autograd: the gradient of sum(score * dscore) at q'
    qr = qp.double().requires_grad_(True)
    v = vp.double().view(N, P, mid)[img]
    x = torch.relu(v * qr[:, None, :] if mode == 1 else v + qr[:, None, :])
    ((x @ wx.double().t()).permute(0, 2, 1) * ds.double()).sum().backward()
    d = lambda t: t.to(DEV)
    args = (d(ds), d(vp), d(qp), d(wx), d(order), d(offsets), N, B, P, mode)
    dq_part, NT = ops.att_attr_dq_grouped(*args)
    dq = ops.sum_parts(dq_part, torch.empty(B, mid, device=DEV), B, NT, mid)
    torch.cuda.synchronize()
    tag = f"{N,B,P,mid,G} mode {mode} {kind}"
    check(f"att_attr_dq_grouped dq' {tag}", dq, qr.grad, 1e-5)                 # every element, of the largest entry
    # the kernel it derives from, at p = 0: the same bits
    _dvp, dq_train, _dwx, NT_train = ops.att_score_grouped_bwd(*args, 0.0, 0)
    assert NT == NT_train and torch.equal(dq_part, dq_train)
    # a float16 v': the fp32 form on the widened values, bit for bit
    vh = d(vp).half()
    part_h, _ = ops.att_attr_dq_grouped(d(ds), vh, *args[2:])
    part_w, _ = ops.att_attr_dq_grouped(d(ds), vh.float(), *args[2:])
    torch.cuda.synchronize()
    assert torch.equal(part_h, part_w)
    # '|' is refused, with the reason
    with pytest.raises(VqaHipError, match="identically zero"):
        ops.att_attr_dq_grouped(d(ds), d(vp), d(qp), d(torch.randn(G, 2 * mid, generator=g)), d(order), d(offsets), N, B, P, 2)
    # questions that are not listed keep what the output held: un-list the questions of the first image that has some
    first = int(img.min())
    cut = offsets.clone()
    cut[:first + 1] = offsets[first + 1]
    kept = torch.full((B * NT, mid), 7.0, device=DEV)
    ops.att_attr_dq_grouped(d(ds), d(vp), d(qp), d(wx), d(order), d(cut), N, B, P, mode, dq_part=kept)
    torch.cuda.synchronize()
    unlisted = d(img == first)
    kept, full = kept.view(B, NT, mid), dq_part.view(B, NT, mid)
    assert bool(unlisted.any()) and bool((kept[unlisted] == 7.0).all()) and torch.equal(kept[~unlisted], full[~unlisted])


# ----------------------------------------------------------------------------- kernel B: the embedding stage
@pytest.mark.parametrize("two", [False, True])
@pytest.mark.parametrize("B,T,E,V", [(3, 5, 12, 50), (2, 1, 300, 40), (5, 7, 20, 30), (4, 14, 302, 60)])
def test_embed_attr_matches_float64(B, T, E, V, two):
    ops = _ops()
    g = torch.Generator().manual_seed(B * 100 + T * 10 + E + int(two))
    emb = torch.randn(V, E, generator=g)
    q = torch.randint(0, V, (B, T), generator=g)
    q_len = torch.randint(1, T + 1, (B,), generator=g)
    q_len[0], q_len[-1] = T, 1                                      # ragged, 1 and T included (B >= 2)
    q[0, 0] = V                                                     # one id outside the vocabulary, inside its question
    x = torch.tanh(torch.randn(T, B, E, generator=g))
    dx0 = torch.randn(T * B, E, generator=g)
    dx1 = torch.randn(T * B, E, generator=g) if two else None
    dx = (dx0 + dx1 if two else dx0).view(T, B, E)
    want = W.words_closed_form(emb, q, x.permute(1, 0, 2), dx.permute(1, 0, 2), q_len)
    d = lambda t: None if t is None else t.to(DEV)
    out = torch.full((B, T), 7.0, device=DEV)
    ops.embed_attr(d(q), d(emb), d(x), d(dx0), d(dx1), d(q_len), out=out)
    torch.cuda.synchronize()
    check(f"embed_attr {B,T,E,V} dx x {1 + int(two)}", out, want, 3e-6)
    dead = d((torch.arange(T)[None, :] >= q_len[:, None]) | (q >= V))
    assert bool(dead.any()) and bool((out[dead] == 0.0).all()) and float(out[0, 0]) == 0.0
    assert bool((out[~dead] != 7.0).all())                          # every element is written
    # the scalar form on the same values (a misaligned dx0, then a misaligned table): the same bits.  E % 4 != 0 is scalar
    # already, and the check still holds
    for which in ("dx0", "emb"):
        a = dict(emb=d(emb), dx0=d(dx0))
        a[which] = _off_by_one_float(a[which])
        again = ops.embed_attr(d(q), a["emb"], d(x), a["dx0"], d(dx1), d(q_len))
        torch.cuda.synchronize()
        assert torch.equal(again, out), which


# ----------------------------------------------------------------------------- the whole path
def _model(case, do_option="+", compute_dtype="fp32"):
    sd = case["sd"] if "sd" in case else case["golden"].sd
    V = case["V"] if "V" in case else case["golden"].meta["V"]
    m = build(case["cfg"], V, sd, compute_dtype).eval()
    return m, m.encode_images(case["v"].to(DEV))


def _stage_parity(tag, case, do_option, got, stages, T):
    """words and the stages against the float64 reference for the answers `got` explains; prints and returns the errors."""
    sd = case["sd"] if "sd" in case else case["golden"].sd
    answers = got.answers.tolist()
    if "golden" in case:
        full, att, _cls = W.fixture_reference(do_option, answers)
    else:
        full, att, _cls = W.reference_parts(sd, do_option, case["vn"], case["q"], case["q_len"], case["img"], answers, case["grid"],
                                            case["cfg"]["text"]["bidirectional"])
    scale = math.sqrt(max(T, 5) / 5)
    e_words = rel(got.words, full["words"])
    e_dqf = rel(stages["dqf"], full["dqf"])
    e_dx = rel(stages["dx"].permute(1, 0, 2), full["dx"])
    line = (f"[parity-words] {tag}: words max|err|/max|ref| = {e_words:.3e} (bound {WORDS_BOUND * scale:.1e}), max|words| "
            f"{float(full['words'].abs().max()):.3e}; dqf {e_dqf:.3e}, dx {e_dx:.3e}")
    if do_option != "|":
        e_dq = rel(stages["dq_att"], att["dqp"])
        line += f"; dq_att max|err|/max|ref| = {e_dq:.3e} (bound {DQ_BOUND:.0e}), max|dq_att| {float(att['dqp'].abs().max()):.3e}"
    print(line)
    if do_option != "|":
        assert float(att["dqp"].abs().max()) > 0 and e_dq < DQ_BOUND
    assert e_words < WORDS_BOUND * scale
    assert e_dqf < WORDS_BOUND * scale and e_dx < WORDS_BOUND * scale
    return e_words


@pytest.mark.parametrize("do_option", ["+", "*", "|"])
def test_explain_words_matches_autograd_on_fixtures(do_option):
    f = R.fixture_case(do_option)
    assert W.case_near_zero(f, do_option) == 0                      # the precondition of the ReLU indicators
    m, feats = _model(f)
    name = R.FIXTURES[do_option]
    q, ql, img = f["q"].to(DEV), f["q_len"].to(DEV), list(R.IMAGE_INDEX)
    B, T = f["q"].shape
    A, eng = f["cfg"]["max_answers"], m._engine
    stages = {}
    got = m.explain_words(feats, q, ql, img, _stages=stages)
    torch.cuda.synchronize()
    assert isinstance(got, WordAttribution) and got.words.shape == (B, T) and got.words.dtype == torch.float32
    assert not got.words.requires_grad and m._last_ctx is None
    assert stages["dq_att"].shape == (B, eng.mid) and stages["dqf"].shape == (B, eng.Q) and stages["dx"].shape == (T, B, eng.E)
    # maps, answers, logits: explain's bits
    att = m.explain(feats, q, ql, img)
    assert torch.equal(got.maps, att.maps) and torch.equal(got.answers, att.answers) and torch.equal(got.logits, att.logits)
    pad = (torch.arange(T)[None, :] >= f["q_len"][:, None]).to(DEV)
    assert bool(pad.any()) and bool((got.words[pad] == 0.0).all())
    if do_option == "|":
        # nothing ran for the attention path: no kernel A, no q_lin product, and the stage is the zeros the engine reports;
        # dqf is then the classifier product alone, which _stage_parity holds against the float64 gradient
        assert stages["attention_path"] == () and bool((stages["dq_att"] == 0.0).all())
    else:
        assert stages["attention_path"] == ("att_attr_dq_grouped", "sum_parts", "q_lin")
        assert float(stages["dq_att"].abs().max()) > 0
    _stage_parity(f"{name} arg-max", f, do_option, got, stages, T)
    # given columns: a list, and an out-of-range CUDA entry (a row of zeros, as explain's map)
    cols = [(3 * b + 1) % A for b in range(B)]
    stages = {}
    given = m.explain_words(feats, q, ql, img, answers=cols, _stages=stages)
    assert given.answers.tolist() == cols and torch.equal(given.logits, got.logits)
    assert torch.equal(given.maps, m.explain(feats, q, ql, img, answers=cols).maps)
    _stage_parity(f"{name} given columns", f, do_option, given, stages, T)
    bad = torch.tensor(cols, device=DEV)
    bad[2] = A
    zero = m.explain_words(feats, q, ql, img, answers=bad)
    assert float(zero.words[2].abs().max()) == 0.0 and torch.equal(zero.words[:2], given.words[:2])
    assert torch.equal(zero.words[3:], given.words[3:])
    # an empty batch
    none = m.explain_words(feats, q[:0], ql[:0], [])
    assert none.words.shape == (0, T) and none.maps.shape == (0, *feats.grid) and none.logits.shape == (0, A)
    assert m._last_ctx is None and all(p.grad is None for p in m.parameters())


@pytest.mark.parametrize("bidirectional", [True, False])
def test_explain_words_on_the_fused_recurrence(bidirectional):
    """The fixtures have H = 16 (the per-step path); these models have H = 32 and take vqa_lstm_seq_bwd."""
    for T in (6, 1):
        case = W.random_case(bidirectional, T)
        assert W.case_near_zero(case, "+") == 0
        m, feats = _model(case)
        assert m._engine._lstm_schedule()[0] and m._engine.ndir == (2 if bidirectional else 1)
        stages = {}
        got = m.explain_words(feats, case["q"].to(DEV), case["q_len"].to(DEV), case["img"], _stages=stages)
        torch.cuda.synchronize()
        pad = (torch.arange(T)[None, :] >= case["q_len"][:, None]).to(DEV)
        assert bool((got.words[pad] == 0.0).all())
        _stage_parity(f"random H=32 {'bi' if bidirectional else 'uni'}directional T={T}", case, "+", got, stages, T)


def test_fp32x3_a_float16_cache_and_batch_invariance():
    f = R.fixture_case("+")
    q, ql, img = f["q"].to(DEV), f["q_len"].to(DEV), list(R.IMAGE_INDEX)
    B, T = f["q"].shape
    m, feats = _model(f, compute_dtype="fp32x3")
    stages = {}
    got = m.explain_words(feats, q, ql, img, _stages=stages)
    _stage_parity("tiny_plus fp32x3", f, "+", got, stages, T)
    # a float16 cache gives what its widened copy gives, bit for bit
    for do_option in ("+", "*", "|"):
        f = R.fixture_case(do_option)
        m, feats = _model(f)
        q, ql = f["q"].to(DEV), f["q_len"].to(DEV)
        f16 = feats.to(torch.float16)
        a16, a32 = m.explain_words(f16, q, ql, img), m.explain_words(f16.to(torch.float32), q, ql, img)
        assert torch.equal(a16.words, a32.words) and torch.equal(a16.maps, a32.maps) and torch.equal(a16.logits, a32.logits)
        # a split and permuted batch: within the bound of the whole (bit equality is not claimed: the GEMM plans may depend on B)
        a0 = m.explain_words(feats, q, ql, img)
        perm = torch.randperm(B, generator=torch.Generator().manual_seed(3))
        idx = torch.tensor(img)
        h = B // 3
        lo = m.explain_words(feats, q[perm[:h]], ql[perm[:h]], idx[perm[:h]], answers=a0.answers[perm[:h].to(DEV)])
        hi = m.explain_words(feats, q[perm[h:]], ql[perm[h:]], idx[perm[h:]], answers=a0.answers[perm[h:].to(DEV)])
        e = rel(torch.cat([lo.words, hi.words]), a0.words[perm.to(DEV)])
        print(f"[parity-words] {R.FIXTURES[do_option]} split and permuted batch vs whole: words max|diff|/max = {e:.3e}")
        assert e < WORDS_BOUND


def test_forward_and_backward_are_unchanged_after_explain_words():
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
    got = m.explain_words(feats, q, ql, idx)
    torch.cuda.synchronize()
    assert torch.equal(got.logits, m.answer(feats, q, ql, idx))
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
        fresh.explain_words(feats, q, ql, idx)
    with pytest.raises(IndexError):
        m.explain_words(feats, q, ql, idx[:-1] + [feats.N])
