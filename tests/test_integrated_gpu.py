"""GPU: integrated gradients from cached features -- the eight path entry points against float64 (tests/integrated_ref.py) on
inputs whose ReLU pre-activations are exact in fp32, their pairs / half / permuted / split / unlisted forms bit for bit, and
VqaNet.explain_integrated / explain_integrated_pairs on the golden fixtures against the float64 Riemann sum by autograd, against
the brute-force route through explain(), and against themselves under a float16 cache and a lowered workspace cap.
`python -m pytest tests/test_integrated_gpu.py -m gpu -s` prints the measured errors (profiles/integrated_parity.txt)."""
import pytest
import torch

from dl_vqa_amd import ImageFeatures, IntegratedGradients, group_by_image, unique_questions
from tests import attribution_ref as R
from tests import integrated_ref as I
from tests.explain_util import columns, fixture_model as _fixture_model, rel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# 3 images asked by 1, 0 and 5 questions
N, IMG = 3, (2, 2, 0, 2, 2, 2)
B = len(IMG)
POSITIONS = (5, 18, 33)              # a short tile, one position past a tile of 16, two tiles plus one
GLIMPSES = (1, 2)
# dyadic step positions: alpha * v' (+|*) q' is exact in fp32 for v', q' multiples of 1/8 up to 4
ALPHAS = {1: [1 / 2], 3: [1 / 8, 1 / 2, 7 / 8], 8: [(2 * s + 1) / 16 for s in range(8)], 64: [(2 * s + 1) / 128 for s in range(64)]}
# the register kernel's IT = 1..4 ('+' / '*'; '|' takes the general kernel there), then 4, 2 and 1 positions per wave in every mode
MIDS = (256, 512, 768, 1024, 24, 1028, 2052)
BOUND = 3e-6                         # the project's bound for these walks against float64


def _ops():
    from dl_vqa_amd import ops
    return ops


def _expected_path(mode, mid):
    """The launcher's dispatch (csrc/att_score.hip att_score_grouped_pw), restated: 0 = the register kernel."""
    if mode != 2 and mid % 256 == 0 and mid <= 1024:
        return 0
    return 4 if mid <= 1024 else (2 if mid <= 2048 else 1)


def test_the_sizes_reach_every_branch_of_the_launcher():
    ops = _ops()
    reached = set()
    for mid in MIDS:
        for mode in (0, 1, 2):
            path = ops.att_attr_score_grouped_path(mode, mid)
            assert path == _expected_path(mode, mid)
            reached.add(("register", mid // 256, mode) if path == 0 else ("general", path, mode))
    assert {r for r in reached if r[0] == "register"} == {("register", it, mode) for it in (1, 2, 3, 4) for mode in (0, 1)}
    assert {r for r in reached if r[0] == "general"} == {("general", pw, mode) for pw in (4, 2, 1) for mode in (0, 1, 2)}


def _eighths(g, *shape):
    """Multiples of 1/8 in [-4, 4]."""
    return torch.randint(-32, 33, shape, generator=g).float() / 8


def _operands(mid, mode, P, G, S, seed):
    g = torch.Generator().manual_seed(seed)
    vp, qp = _eighths(g, N * P, mid), _eighths(g, B, mid)
    wx = _eighths(g, G, 2 * mid if mode == 2 else mid)
    bx = torch.randn(G, generator=g)
    r1, ds = torch.randn(B, S, P, generator=g), torch.randn(B, S, G, P, generator=g)
    return g, vp, qp, wx, bx, r1, ds, torch.tensor(ALPHAS[S], dtype=torch.float32)


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("mid", MIDS)
def test_path_kernels_match_float64(mid, mode):
    """Each (P, G, S) of the issue's table: scores and maps against float64 on every element, then the bit-for-bit forms."""
    ops = _ops()
    d = lambda t: t.to(DEV)
    img = torch.tensor(IMG)
    order, offsets = group_by_image(img, N)
    path = ops.att_attr_score_grouped_path(mode, mid)
    assert path == _expected_path(mode, mid)
    worst_s = worst_a = 0.0
    for P in POSITIONS:
        for G in GLIMPSES:
            for S in ALPHAS:
                g, vp, qp, wx, bx, r1, ds, al = _operands(mid, mode, P, G, S, seed=mid * 100 + mode * 10 + P + G + S)
                scale = 1.0 / S
                tag = f"mid {mid} mode {mode} path {path} P {P} G {G} S {S}"
                score = torch.full((B, S, G, P), 7.0, device=DEV)
                ops.att_path_score_grouped(d(vp), d(qp), d(wx), d(bx), d(al), d(order), d(offsets), N, B, P, mode, out=score)
                out = torch.full((B, P), 7.0, device=DEV)
                ops.att_path_attr_grouped(d(r1), d(ds), d(vp), d(qp), d(wx), d(al), scale, d(order), d(offsets), N, B, P, mode,
                                          out=out)
                torch.cuda.synchronize()
                want_s = I.path_scores(vp.view(N, P, mid), qp, wx, bx, img, mode, al)
                want_a = I.path_attr(r1, ds, vp.view(N, P, mid), qp, wx, img, mode, al, scale)
                es, ea = rel(score, want_s), rel(out, want_a)                    # every element: nothing keeps the 7.0
                worst_s, worst_a = max(worst_s, es), max(worst_a, ea)
                assert es <= BOUND, f"path scores {tag}: {es}"
                assert ea <= BOUND, f"path attribution {tag}: {ea}"
                if mode == 2:                                                    # '|' reads no q' in the attribution
                    noq = ops.att_path_attr_grouped(d(r1), d(ds), d(vp), None, d(wx), d(al), scale, d(order), d(offsets), N, B, P,
                                                    mode)
                    assert torch.equal(noq, out)
                # questions that are not listed keep what the outputs held: un-list the questions of image 0
                cut = offsets.clone()
                cut[:1] = offsets[1]
                kept_s, kept_a = torch.full((B, S, G, P), 7.0, device=DEV), torch.full((B, P), 7.0, device=DEV)
                ops.att_path_score_grouped(d(vp), d(qp), d(wx), d(bx), d(al), d(order), d(cut), N, B, P, mode, out=kept_s)
                ops.att_path_attr_grouped(d(r1), d(ds), d(vp), d(qp), d(wx), d(al), scale, d(order), d(cut), N, B, P, mode,
                                          out=kept_a)
                unl = d(img == 0)
                assert bool(unl.any()) and bool((kept_s[unl] == 7.0).all()) and bool((kept_a[unl] == 7.0).all())
                assert torch.equal(kept_s[~unl], score[~unl]) and torch.equal(kept_a[~unl], out[~unl])
                # the pairs form over a table of distinct questions: the plain form on qp[qrow], bit for bit
                table = _eighths(g, 3, mid)
                qrow = torch.randint(0, 3, (B,), generator=g)
                qr = d(qrow.to(torch.int32))
                sp = ops.att_path_score_grouped(d(vp), d(table), d(wx), d(bx), d(al), d(order), d(offsets), N, B, P, mode, qrow=qr)
                se = ops.att_path_score_grouped(d(vp), d(table[qrow]), d(wx), d(bx), d(al), d(order), d(offsets), N, B, P, mode)
                ap = ops.att_path_attr_grouped(d(r1), d(ds), d(vp), d(table), d(wx), d(al), scale, d(order), d(offsets), N, B, P,
                                               mode, qrow=qr)
                ae = ops.att_path_attr_grouped(d(r1), d(ds), d(vp), d(table[qrow]), d(wx), d(al), scale, d(order), d(offsets), N,
                                               B, P, mode)
                assert torch.equal(sp, se) and torch.equal(ap, ae)
                # a float16 v' (multiples of 1/8 are halves exactly, so perturb it first): the fp32 form on the widened values
                vh = (d(vp) + 0.013).half()
                for q_, row in ((d(qp), None), (d(table), qr)):
                    s16 = ops.att_path_score_grouped(vh, q_, d(wx), d(bx), d(al), d(order), d(offsets), N, B, P, mode, qrow=row)
                    s32 = ops.att_path_score_grouped(vh.float(), q_, d(wx), d(bx), d(al), d(order), d(offsets), N, B, P, mode,
                                                     qrow=row)
                    a16 = ops.att_path_attr_grouped(d(r1), d(ds), vh, q_, d(wx), d(al), scale, d(order), d(offsets), N, B, P, mode,
                                                    qrow=row)
                    a32 = ops.att_path_attr_grouped(d(r1), d(ds), vh.float(), q_, d(wx), d(al), scale, d(order), d(offsets), N, B,
                                                    P, mode, qrow=row)
                    assert torch.equal(s16, s32) and torch.equal(a16, a32)
                # a permuted batch permutes the rows; a batch split in two concatenates them
                perm = torch.randperm(B, generator=g)
                po, pf = group_by_image(img[perm], N)
                s_p = ops.att_path_score_grouped(d(vp), d(qp[perm]), d(wx), d(bx), d(al), d(po), d(pf), N, B, P, mode)
                a_p = ops.att_path_attr_grouped(d(r1[perm]), d(ds[perm]), d(vp), d(qp[perm]), d(wx), d(al), scale, d(po), d(pf), N,
                                                B, P, mode)
                assert torch.equal(s_p, score[d(perm)]) and torch.equal(a_p, out[d(perm)])
                parts_s, parts_a = [], []
                for lo, hi in ((0, 2), (2, B)):
                    so, sf = group_by_image(img[lo:hi], N)
                    parts_s.append(ops.att_path_score_grouped(d(vp), d(qp[lo:hi]), d(wx), d(bx), d(al), d(so), d(sf), N, hi - lo,
                                                              P, mode))
                    parts_a.append(ops.att_path_attr_grouped(d(r1[lo:hi]), d(ds[lo:hi]), d(vp), d(qp[lo:hi]), d(wx), d(al), scale,
                                                             d(so), d(sf), N, hi - lo, P, mode))
                torch.cuda.synchronize()
                assert torch.equal(torch.cat(parts_s), score) and torch.equal(torch.cat(parts_a), out)
    print(f"[parity-integrated] mid {mid} mode {mode} path {path}: over P {POSITIONS} x G {GLIMPSES} x S {tuple(ALPHAS)}, "
          f"max|err|/max|ref| path scores {worst_s:.3e}, path attribution {worst_a:.3e} (bound {BOUND:.0e})")


def test_one_step_at_alpha_one_is_the_grouped_forward_and_attribution():
    """S = 1, alpha = 1, scale = 1: x = 1 * v' is v', so the path kernels return the bits of the kernels they extend."""
    ops = _ops()
    d = lambda t: t.to(DEV)
    img = torch.tensor(IMG)
    order, offsets = group_by_image(img, N)
    one = torch.ones(1, device=DEV)
    for mid, mode in ((1024, 0), (512, 1), (24, 2), (1028, 1)):
        g, vp, qp, wx, bx, r1, ds, _ = _operands(mid, mode, 18, 2, 1, seed=mid + mode)
        vp = vp + 0.1 * torch.randn(vp.shape, generator=g)
        s1 = ops.att_path_score_grouped(d(vp), d(qp), d(wx), d(bx), one, d(order), d(offsets), N, B, 18, mode)
        s0 = ops.att_score_grouped_fwd(d(vp), d(qp), d(wx), d(bx), d(order), d(offsets), N, B, 18, mode)
        a1 = ops.att_path_attr_grouped(d(r1), d(ds), d(vp), d(qp), d(wx), one, 1.0, d(order), d(offsets), N, B, 18, mode)
        a0 = ops.att_attr_score_grouped(d(r1[:, 0]).contiguous(), d(ds[:, 0]).contiguous(), d(vp), d(qp), d(wx), d(order),
                                        d(offsets), N, B, 18, mode)
        assert torch.equal(s1[:, 0], s0) and torch.equal(a1, a0)


def test_scale_rows():
    ops = _ops()
    g = torch.Generator().manual_seed(5)
    x = torch.randn(3 * 5, 11, generator=g)
    al = torch.tensor(ALPHAS[3] + [1 / 4, 3 / 4], dtype=torch.float32)
    got = ops.att_path_scale_rows(x.to(DEV), al.to(DEV), 7)
    want = x.clone()
    want[:, :7] *= al.repeat(3)[:, None]
    assert torch.equal(got.cpu(), want)


# ----------------------------------------------------------------------------- the whole path on the golden fixtures
WHOLE_PATH = 2e-4                    # the family's whole-path bound against float64, of max|ref| (tests/test_attribution_gpu.py)


def _parity(tag, ig, do_option, steps):
    ref = I.fixture_reference(do_option, ig.answers.tolist(), steps)
    e = rel(ig.maps.reshape(ref.shape[0], -1), ref)
    print(f"[parity-integrated] {tag} S={steps}: maps max|err|/max|ref| = {e:.3e} (bound {WHOLE_PATH:.0e}), max|IG| "
          f"{float(ref.abs().max()):.3e}")
    assert e < WHOLE_PATH
    # the device's completeness gap is the float64 gap of the same Riemann sum: that it matches, not that it is small
    gap64 = I.fixture_gap(do_option, ig.answers.tolist(), ref)
    dg = float((ig.completeness_gap().cpu() - gap64).abs().max())
    print(f"[parity-integrated] {tag} S={steps}: completeness gap max|device - float64| = {dg:.3e} (bound "
          f"{WHOLE_PATH * float(ref.abs().max()):.3e}), max|gap| {float(gap64.abs().max()):.3e}")
    assert dg < WHOLE_PATH * float(ref.abs().max())
    return ref


def _brute_force(m, feats, q, ql, img, answers, steps):
    """The route through the public API: explain() with the same columns on the cache scaled by alpha_s, divided by alpha_s,
    averaged (float64 on the host)."""
    total = 0
    for a in I.alphas64(steps).tolist():
        scaled = ImageFeatures(feats.vn * a, feats.vprime * a, feats.grid, m)
        total = total + m.explain(scaled, q, ql, img, answers=answers).maps.double().cpu() / a
    return total / steps


@pytest.mark.parametrize("compute_dtype", ["fp32", "fp32x3"])
@pytest.mark.parametrize("do_option", ["+", "*", "|"])
def test_explain_integrated_matches_the_riemann_sum_on_fixtures(do_option, compute_dtype):
    f, m, feats = _fixture_model(do_option, compute_dtype)
    name = f"{R.FIXTURES[do_option]} {compute_dtype}"
    q, ql, img = f["q"].to(DEV), f["q_len"].to(DEV), list(R.IMAGE_INDEX)
    Bq, A = len(img), f["cfg"]["max_answers"]
    qu, qlu, qidx = unique_questions(f["q"], f["q_len"])
    qfeats = m.encode_questions(qu.to(DEV), qlu.to(DEV))
    logits = m.answer(feats, q, ql, img)
    zeroed = ImageFeatures(torch.zeros_like(feats.vn), torch.zeros_like(feats.vprime), feats.grid, m)
    logits0 = m.answer(zeroed, q, ql, img)
    cols = columns(Bq, A)
    for steps in (8, 16):
        ig = m.explain_integrated(feats, q, ql, img, steps=steps)
        torch.cuda.synchronize()
        assert isinstance(ig, IntegratedGradients) and ig.maps.shape == (Bq, *feats.grid) and ig.maps.dtype == torch.float32
        assert ig.answers.dtype == torch.int64 and ig.baseline_logits.shape == (Bq,) and not ig.maps.requires_grad
        assert torch.equal(ig.logits, logits)
        assert torch.equal(ig.answers, m.predict(feats, q, ql, img, k=1).indices[:, 0])
        assert torch.equal(ig.baseline_logits, logits0.gather(1, ig.answers[:, None])[:, 0])
        ref = _parity(f"{name} explain_integrated arg-max", ig, do_option, steps)
        given = m.explain_integrated(feats, q, ql, img, answers=cols, steps=steps)
        assert given.answers.tolist() == cols and torch.equal(given.logits, logits)
        assert torch.equal(given.baseline_logits, logits0.gather(1, given.answers[:, None])[:, 0])
        _parity(f"{name} explain_integrated given columns", given, do_option, steps)
        # the same pairs from the two caches
        pairs = m.explain_integrated_pairs(feats, qfeats, img, qidx, steps=steps)
        assert torch.equal(pairs.logits, m.answer_pairs(feats, qfeats, img, qidx))
        assert torch.equal(pairs.baseline_logits,
                           m.answer_pairs(zeroed, qfeats, img, qidx).gather(1, pairs.answers[:, None])[:, 0])
        _parity(f"{name} explain_integrated_pairs arg-max", pairs, do_option, steps)
        _parity(f"{name} explain_integrated_pairs given columns",
                m.explain_integrated_pairs(feats, qfeats, img, qidx, answers=cols, steps=steps), do_option, steps)
        # the brute-force route through explain()
        brute = _brute_force(m, feats, q, ql, img, ig.answers.tolist(), steps)
        eb, ed = rel(brute.reshape(Bq, -1), ref), rel(ig.maps.reshape(Bq, -1), brute.reshape(Bq, -1))
        print(f"[parity-integrated] {name} S={steps}: {steps} explain() calls on scaled caches vs float64 {eb:.3e} (bound "
              f"{WHOLE_PATH:.0e}); explain_integrated vs that route {ed:.3e}")
        assert eb < WHOLE_PATH
    # a CUDA column outside [0, A): a zero map and a zero baseline, the other rows untouched
    bad = torch.tensor(cols, device=DEV)
    bad[2] = A
    zero = m.explain_integrated(feats, q, ql, img, answers=bad, steps=16)
    assert float(zero.maps[2].abs().max()) == 0.0 and float(zero.baseline_logits[2]) == 0.0
    assert torch.equal(zero.maps[:2], given.maps[:2]) and torch.equal(zero.maps[3:], given.maps[3:])
    # an empty batch
    none = m.explain_integrated(feats, q[:0], ql[:0], [], steps=8)
    assert none.maps.shape == (0, *feats.grid) and none.answers.dtype == torch.int64 and none.baseline_logits.shape == (0,)
    none = m.explain_integrated_pairs(feats, qfeats, [], [])
    assert none.maps.shape == (0, *feats.grid) and none.logits.shape == (0, A)
    assert m._last_ctx is None and all(p.grad is None for p in m.parameters())


@pytest.mark.parametrize("do_option", ["+", "*", "|"])
def test_float16_cache_chunks_and_order_are_bit_for_bit(do_option):
    f, m, feats = _fixture_model(do_option)
    q, ql, img = f["q"].to(DEV), f["q_len"].to(DEV), list(R.IMAGE_INDEX)
    Bq = len(img)
    qu, qlu, qidx = unique_questions(f["q"], f["q_len"])
    qfeats = m.encode_questions(qu.to(DEV), qlu.to(DEV))
    same = lambda a, b: torch.equal(a.maps, b.maps) and torch.equal(a.logits, b.logits) and torch.equal(a.answers, b.answers) \
        and torch.equal(a.baseline_logits, b.baseline_logits)
    # a float16 cache gives what its widened copy gives
    f16 = feats.to(torch.float16)
    f32 = f16.to(torch.float32)
    assert same(m.explain_integrated(f16, q, ql, img, steps=8), m.explain_integrated(f32, q, ql, img, steps=8))
    assert same(m.explain_integrated_pairs(f16, qfeats, img, qidx, steps=8), m.explain_integrated_pairs(f32, qfeats, img, qidx, steps=8))
    # a workspace cap that holds 3 questions: 3 chunks of the 7, the unchunked maps
    whole = m.explain_integrated(feats, q, ql, img, steps=8)
    eng = m._engine
    cap = 3 * 8 * feats.vn.shape[1] * (3 * eng.G + 1) * 4
    assert eng.integrated_rows(feats.vn.shape[1], 8, cap) == 3 and Bq > 6
    assert same(m.explain_integrated(feats, q, ql, img, steps=8, _ig_bytes=cap), whole)
    assert same(m.explain_integrated(feats, q, ql, img, steps=8, _ig_bytes=1), whole)                     # one question per chunk
    pw = m.explain_integrated_pairs(feats, qfeats, img, qidx, steps=8)
    assert same(m.explain_integrated_pairs(feats, qfeats, img, qidx, steps=8, _ig_bytes=cap), pw)
    # a permuted batch permutes the rows; a split batch concatenates them
    perm = torch.randperm(Bq, generator=torch.Generator().manual_seed(3))
    a1 = m.explain_integrated(feats, q[perm.to(DEV)], ql[perm.to(DEV)], [img[i] for i in perm.tolist()], steps=8)
    assert torch.equal(a1.maps, whole.maps[perm.to(DEV)]) and torch.equal(a1.baseline_logits, whole.baseline_logits[perm.to(DEV)])
    lo, hi = m.explain_integrated(feats, q[:2], ql[:2], img[:2], steps=8), m.explain_integrated(feats, q[2:], ql[2:], img[2:], steps=8)
    assert torch.equal(torch.cat([lo.maps, hi.maps]), whole.maps)
    assert m._last_ctx is None and all(p.grad is None for p in m.parameters())
