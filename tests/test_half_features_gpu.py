"""GPU: float16 image-feature caches.  One rule: a float16 cache is the fp32 cache with each tensor rounded once to nearest
even, and every consumer computes in fp32 on the widened values.  So (1) the converter has the bits of torch's .half(), and
(2) every kernel that reads a cache -- vqa_gather_rows_drop, vqa_att_apply_gather_fwd / _dscore, vqa_att_score_grouped_fwd /
_pairs_fwd -- and every public call on top of them gives on a float16 operand, bit for bit, what it gives on the fp32 tensor
holding the same values.  Every comparison here is torch.equal; the one test with a bound (the last) measures how far the
answers from a float16 cache are from the answers from the unrounded fp32 cache.

`python -m tests.test_half_features_gpu` prints that measurement (profiles/half_features_parity.txt)."""
import pytest
import torch

from dl_vqa_amd import ImageFeatures, group_by_image
from tests.golden_util import TINY_CASES, Golden, tiny_cfg
from tests.test_feature_train_gpu import BANK_INDEX, _bank_batch, _encode, features_step
from tests.test_model_gpu import build
from tests.test_shared_train_gpu import _full224_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 0x5EED0FBA2C0FFEE


def _ops():
    from dl_vqa_amd import ops
    return ops


def _bits(t):
    return t.contiguous().view(torch.int16)


# ----------------------------------------------------------------------------- vqa_float_to_half
NAN = float("nan")
SPECIALS = [0.0, -0.0,
            2.0 ** -24, -2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -25, 3.0 * 2.0 ** -25,      # fp16 subnormals and the ties around them
            2.0 ** -14, 2.0 ** -14 - 2.0 ** -24, 2.0 ** -14 - 2.0 ** -25,                # smallest normal, largest subnormal, a tie
            1e-40, -1e-40, 1.4e-45,                                                       # fp32 subnormals
            65504.0, 65519.0, 65520.0, -65519.0, -65520.0, 1e10,                          # the overflow threshold: 65520 -> inf
            float("inf"), float("-inf"), NAN,
            1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 2.0 ** -11), 1 + 2.0 ** -11 + 2.0 ** -23]


def _check_to_half(x):
    """ops.to_half(x) has the bits of torch's .half(), the host's and the device's."""
    ops = _ops()
    xd = x.to(DEV)
    buf = torch.full((x.numel() + 16,), 7.0, dtype=torch.float16, device=DEV)
    out = ops.to_half(xd, out=buf[8:8 + x.numel()])
    got = ops.to_half(xd)
    torch.cuda.synchronize()
    assert got.dtype == torch.float16 and got.shape == x.shape and out.data_ptr() == buf.data_ptr() + 16
    assert torch.equal(_bits(got), _bits(x.half()).to(DEV))
    assert torch.equal(_bits(got), _bits(xd.half()))
    assert torch.equal(_bits(out), _bits(got))
    assert bool((buf[:8] == 7).all()) and bool((buf[8 + x.numel():] == 7).all())         # nothing outside out
    return got


@pytest.mark.parametrize("n", [1, 7, 8, 9, 1027])
def test_to_half_has_the_bits_of_torch_half_on_random_normals(n):
    g = torch.Generator().manual_seed(n)
    _check_to_half(torch.randn(n, generator=g))
    _check_to_half(torch.randn(n, generator=g) * 1e-6)                                    # down into the fp16 subnormals
    _check_to_half(torch.randn(n, generator=g) * 3e4)                                     # up across the overflow threshold


def test_to_half_rounds_specials_and_exact_ties_as_torch_half():
    x = torch.tensor(SPECIALS, dtype=torch.float32)
    assert x.numel() > 24                                             # the vector path and the scalar tail both see specials
    for shift in (0, 3, 11):
        _check_to_half(torch.roll(x, shift))
    h = _check_to_half(x).cpu()
    at = lambda v: h[SPECIALS.index(v)]
    assert float(at(1 + 2.0 ** -11)) == 1.0                           # a tie: to the even mantissa, down
    assert float(at(1 + 3 * 2.0 ** -11)) == 1 + 2.0 ** -9             # a tie: to the even mantissa, up
    assert float(at(1 + 2.0 ** -11 + 2.0 ** -23)) == 1 + 2.0 ** -10   # just above a tie: up
    assert float(at(65519.0)) == 65504.0 and float(at(65520.0)) == float("inf") and float(at(-65520.0)) == float("-inf")
    assert float(at(2.0 ** -25)) == 0.0 and float(at(1.5 * 2.0 ** -25)) == 2.0 ** -24     # subnormals kept, ties to even
    assert float(at(2.0 ** -14 - 2.0 ** -24)) == 2.0 ** -14 - 2.0 ** -24
    assert bool(torch.isnan(at(NAN))) and bool(torch.signbit(h[1])) and float(h[1]) == 0.0 and bool(torch.signbit(at(-1e-40)))


def test_half_to_float_to_half_round_trips_every_fp16_value():
    """All 65 536 bit patterns: every one that is a value (zeros, subnormals, normals, infinities) comes back with its bits;
    a NaN comes back a NaN of the same sign (a conversion may quiet a signalling NaN, so its payload is not pinned)."""
    ops = _ops()
    table = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).to(DEV)
    h = table.view(torch.float16)
    wide = ops.half_to_float(h)
    back = ops.to_half(wide)
    torch.cuda.synchronize()
    nan = torch.isnan(h)
    assert int(nan.sum()) == 2 * 1023 and torch.equal(torch.isnan(wide), nan) and torch.equal(torch.isnan(back), nan)
    assert torch.equal(_bits(back)[~nan], table[~nan])
    assert torch.equal(wide[~nan], h.float()[~nan])                   # widening is exact
    assert torch.equal(_bits(back)[nan] < 0, table[nan] < 0)
    print(f"[half] NaN payloads kept by the round trip: {int((_bits(back)[nan] == table[nan]).sum())} of {int(nan.sum())}")


# ----------------------------------------------------------------------------- vqa_gather_rows_drop on a float16 bank
def _half_bank(M, row_len, gen, off=0):
    """A float16 bank [M, row_len] that starts `off` halves into its allocation."""
    flat = torch.zeros(M * row_len + 8, dtype=torch.float16)
    flat[off:off + M * row_len] = torch.randn(M * row_len, generator=gen).half()
    return flat.to(DEV)[off:off + M * row_len].view(M, row_len)


def _gather_half(n, M, row_len, p, rows=None, src_off=0, dst_off=0):
    ops = _ops()
    g = torch.Generator().manual_seed(n * 31 + M * 7 + row_len)
    bank = _half_bank(M, row_len, g, src_off)
    assert bank.data_ptr() % 16 == 2 * src_off and bank.is_contiguous()
    rows = torch.randint(0, M, (n,), generator=g) if rows is None else torch.as_tensor(rows)
    rows_d = rows.to(torch.int32).to(DEV)
    want = ops.gather_rows_drop(bank.float(), rows_d, p, SEED)        # the fp32 kernel on the widened bank
    buf = torch.full((n * row_len + 8,), 7.0, device=DEV)
    dst = buf[dst_off:dst_off + n * row_len].view(n, row_len)
    out = ops.gather_rows_drop(bank, rows_d, p, SEED, out=dst)
    fresh = ops.gather_rows_drop(bank, rows_d, p, SEED)
    torch.cuda.synchronize()
    assert out.data_ptr() == dst.data_ptr() and fresh.dtype == torch.float32
    assert torch.equal(dst, want) and torch.equal(fresh, want)
    assert bool((buf[:dst_off] == 7).all()) and bool((buf[dst_off + n * row_len:] == 7).all())      # nothing outside dst
    inside = ((rows >= 0) & (rows < M)).to(DEV)
    assert float(dst[~inside].abs().max() if bool((~inside).any()) else 0.0) == 0.0
    if p == 0:
        assert torch.equal(dst[inside], bank.float()[rows_d[inside].long()])
    return dst


@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("n,M,row_len", [(3, 5, 224), (1, 1, 8), (4, 6, 12), (4, 6, 111), (2, 3, 173056)])
def test_gather_rows_drop_half_bank_has_the_bits_of_the_fp32_kernel(n, M, row_len, p):
    _gather_half(n, M, row_len, p)


@pytest.mark.parametrize("p", [0.0, 0.3])
def test_gather_rows_drop_half_bank_repeats_bad_rows_and_misalignment(p):
    dst = _gather_half(6, 4, 40, p, rows=[3, 3, 0, 3, 1, 0])                               # repeated rows
    assert torch.equal(dst[0], dst[1]) and torch.equal(dst[0], dst[3])
    dst = _gather_half(5, 4, 40, p, rows=[1, 4, 0, -1, 3])                                 # rows -1 and M: zeros
    assert float(dst[1].abs().max()) == 0.0 and float(dst[3].abs().max()) == 0.0 and float(dst[0].abs().max()) > 0
    a = _gather_half(5, 7, 64, p, rows=[6, 2, 2, 0, 5])                                    # the quad path
    b = _gather_half(5, 7, 64, p, rows=[6, 2, 2, 0, 5], src_off=1)                         # the bank one half off: scalar path
    c = _gather_half(5, 7, 64, p, rows=[6, 2, 2, 0, 5], dst_off=1)                         # dst 4 bytes off: scalar path
    d = _gather_half(5, 7, 64, p, rows=[6, 2, 2, 0, 5], src_off=4)                         # 8-byte aligned, not 16: quad path
    assert c.data_ptr() % 16 == 4 and torch.equal(a, b) and torch.equal(a, c) and torch.equal(a, d)


# ----------------------------------------------------------------------------- vqa_att_apply_gather_fwd / _dscore on a float16 vn
def _apply_case(N, B, P, C, G, asked=None, vn_off=0):
    g = torch.Generator().manual_seed(B * 1000 + P + C)
    vn = _half_bank(N, P * C, g, vn_off).view(N, P, C)
    score = (torch.randn(B, G, P, generator=g) * 2).to(DEV)
    ld = G * C + 12
    dout = torch.randn(B, ld, generator=g).to(DEV)
    if asked is None:
        img = torch.randint(0, N, (B,), generator=g)
    else:                                                           # a large bank of which a few rows are asked
        img = torch.tensor(asked)[torch.randint(0, len(asked), (B,), generator=g)]
        img[:len(asked)] = torch.tensor(asked)
    return vn, score, dout, ld, img


def _apply_fwd_both(vn, score, ld, img_d):
    """(probs, out buffer with its sentinels) of the float16 form and of the fp32 form on vn.float()."""
    ops = _ops()
    res = []
    for operand in (vn, vn.float()):
        out = torch.full((score.shape[0], ld), -7.5, device=DEV)
        res.append((ops.att_apply_gather_fwd(score, operand, img_d, out, ld), out))
    torch.cuda.synchronize()
    return res


APPLY_SHAPES = [(2, 7, 676, 256, 2, None), (3, 7, 70, 132, 3, None), (4, 11, 17, 64, 4, None), (3, 5, 1, 8, 1, None),
                (50, 9, 70, 64, 2, (3, 17, 18, 40, 49))]


@pytest.mark.parametrize("N,B,P,C,G,asked", APPLY_SHAPES + [(3, 5, 17, 6, 1, None)])      # the last: C % 4 != 0, scalar kernel
def test_apply_gather_fwd_half_vn_has_the_bits_of_the_fp32_form(N, B, P, C, G, asked):
    vn, score, _, ld, img = _apply_case(N, B, P, C, G, asked)
    img_d = img.to(torch.int32).to(DEV)
    (p16, o16), (p32, o32) = _apply_fwd_both(vn, score, ld, img_d)
    assert torch.equal(p16, p32) and torch.equal(o16, o32)
    assert float(o32[:, :G * C].abs().max()) > 0 and bool((o16[:, G * C:] == -7.5).all())   # written, and only out_ld's G*C


def test_apply_gather_fwd_half_vn_misaligned_and_out_of_range_rows():
    N, B, P, C, G = 4, 11, 17, 64, 4
    vn, score, _, ld, img = _apply_case(N, B, P, C, G)
    img_d = img.to(torch.int32).to(DEV)
    (_, want), _ = _apply_fwd_both(vn, score, ld, img_d)
    # the scalar kernel sums the positions in its own order (4 groups, not 16): its fp32 reference is the fp32 form on a vn
    # that is 4 bytes off, which runs the scalar kernel too
    wide = torch.zeros(vn.numel() + 4, device=DEV)[1:1 + vn.numel()].view(N, P, C).copy_(vn.float())
    assert wide.data_ptr() % 16 == 4
    out_s = torch.full((B, ld), -7.5, device=DEV)
    probs_s = _ops().att_apply_gather_fwd(score, wide, img_d, out_s, ld)
    for off in (1, 2, 4):                                           # 2 and 4 bytes off 8: the scalar kernel; 8 off 16: quads
        shifted, *_ = _apply_case(N, B, P, C, G, vn_off=off)
        assert shifted.data_ptr() % 16 == 2 * off and torch.equal(shifted, vn)
        (p16, o16), (p32, _) = _apply_fwd_both(shifted, score, ld, img_d)
        assert torch.equal(o16, want if off == 4 else out_s) and torch.equal(p16, p32) and torch.equal(p16, probs_s)
    assert float((out_s - want).abs().max()) < 1e-4
    bad = img.clone()
    bad[1], bad[4] = N, -1                                          # left unwritten by both forms
    (p16, o16), (p32, o32) = _apply_fwd_both(vn, score, ld, bad.to(torch.int32).to(DEV))
    keep = torch.ones(B, dtype=torch.bool)
    keep[1] = keep[4] = False
    assert torch.equal(o16, o32) and bool((o16[~keep] == -7.5).all()) and torch.equal(o16[keep], want[keep])
    assert torch.equal(p16[keep], p32[keep])


@pytest.mark.parametrize("N,B,P,C,G,asked", APPLY_SHAPES)
def test_apply_gather_dscore_half_vn_has_the_bits_of_the_fp32_form(N, B, P, C, G, asked):
    ops = _ops()
    vn, score, dout, ld, img = _apply_case(N, B, P, C, G, asked)
    img_d = img.to(torch.int32).to(DEV)
    pr = torch.softmax(score, dim=-1)
    r16, r32 = torch.full((B, G), 7.0, device=DEV), torch.full((B, G), 9.0, device=DEV)
    ds16 = ops.att_apply_gather_dscore(dout, ld, pr, vn, img_d, rowsum=r16)
    ds32 = ops.att_apply_gather_dscore(dout, ld, pr, vn.float(), img_d, rowsum=r32)
    ds16_nors = ops.att_apply_gather_dscore(dout, ld, pr, vn, img_d)
    shifted, *_ = _apply_case(N, B, P, C, G, asked, vn_off=4)       # 8-byte aligned, not 16
    ds16_shift = ops.att_apply_gather_dscore(dout, ld, pr, shifted, img_d)
    torch.cuda.synchronize()
    assert float(ds32.abs().max()) > 0 or P == 1                     # the softmax over one position has no gradient
    assert torch.equal(ds16, ds32) and torch.equal(r16, r32) and torch.equal(ds16_nors, ds32) and torch.equal(ds16_shift, ds32)


# ----------------------------------------------------------------------------- vqa_att_score_grouped_fwd / _pairs_fwd on a float16 v'
@pytest.mark.parametrize("G", [1, 4])
@pytest.mark.parametrize("P", [17, 70])                                # one partial tile; several tiles
@pytest.mark.parametrize("mid", [256, 512, 1024, 132])                 # the register kernel (modes 0, 1); the general kernel
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_grouped_scores_half_vprime_have_the_bits_of_the_fp32_forms(mode, mid, P, G):
    ops = _ops()
    N, B, M = 3, 7, 4
    g = torch.Generator().manual_seed(mid * 10 + P + mode)
    vp = _half_bank(N * P, mid, g)
    qp = torch.randn(B, mid, generator=g).to(DEV)
    qp_u = torch.randn(M, mid, generator=g).to(DEV)
    wx = torch.randn(G, 2 * mid if mode == 2 else mid, generator=g).to(DEV)
    bx = torch.randn(G, generator=g).to(DEV)
    img = torch.randint(0, N - 1, (B,), generator=g)                   # image N-1 has no question
    qrow = torch.randint(0, M, (B,), generator=g).to(torch.int32).to(DEV)
    order, offsets = (t.to(DEV) for t in group_by_image(img, N))
    s16 = ops.att_score_grouped_fwd(vp, qp, wx, bx, order, offsets, N, B, P, mode)
    s32 = ops.att_score_grouped_fwd(vp.float(), qp, wx, bx, order, offsets, N, B, P, mode)
    t16 = ops.att_score_grouped_pairs_fwd(vp, qp_u, qrow, wx, bx, order, offsets, N, B, P, mode)
    t32 = ops.att_score_grouped_pairs_fwd(vp.float(), qp_u, qrow, wx, bx, order, offsets, N, B, P, mode)
    shifted = _half_bank(N * P, mid, torch.Generator().manual_seed(mid * 10 + P + mode), off=4)      # 8-byte aligned, not 16
    s16_shift = ops.att_score_grouped_fwd(shifted, qp, wx, bx, order, offsets, N, B, P, mode)
    torch.cuda.synchronize()
    assert s16.shape == (B, G, P) and float(s32.abs().max()) > 0
    assert torch.equal(s16, s32) and torch.equal(t16, t32) and torch.equal(s16_shift, s32)


# ----------------------------------------------------------------------------- the whole path
def _same_step(a, b):
    (ya, la, ga), (yb, lb, gb) = a, b
    assert torch.equal(ya, yb) and torch.equal(la, lb)
    for k in ga:
        if k.startswith("image."):
            assert ga[k] is None and gb[k] is None, k                  # not in the graph
        else:
            assert ga[k] is not None and torch.equal(ga[k], gb[k]), k


# every tiny fixture in fp32; in fp32x3 those it admits (image.kernel_size == 3: the tiny_k* fixtures run in fp32 only)
WHOLE_PATH_CASES = [(n, dt) for n in TINY_CASES for dt in ("fp32", "fp32x3") if dt == "fp32" or not n.startswith("tiny_k")]


@pytest.mark.parametrize("name,compute_dtype", WHOLE_PATH_CASES)
def test_half_cache_whole_path_is_exact_on_fixtures(name, compute_dtype):
    g = Golden(name)
    cfg = tiny_cfg(g.meta)
    m = build(cfg, g.meta["V"], g.sd, compute_dtype=compute_dtype).eval()
    v, q, ql, a_idx, a_val = _bank_batch(g)
    qd, qld = q.to(DEV), ql.to(DEV)
    f32 = m.encode_images(v.to(DEV))
    f16 = m.encode_images(v.to(DEV), dtype=torch.float16)
    # (1) the bits of the fp32 cache, each tensor rounded once; v' is not recomputed from the rounded vn
    assert f32.dtype == torch.float32 and f16.dtype == torch.float16 and f16.vn.element_size() == 2
    assert f16.vprime.dtype == torch.float16 and f16.grid == f32.grid and f16.N == f32.N
    assert torch.equal(_bits(f16.vn), _bits(f32.vn.half())) and torch.equal(_bits(f16.vprime), _bits(f32.vprime.half()))
    conv = f32.to(torch.float16)
    assert conv is not f32 and torch.equal(_bits(conv.vn), _bits(f16.vn)) and torch.equal(_bits(conv.vprime), _bits(f16.vprime))
    assert f16.to(torch.float16) is f16
    # (2) every consumer: what it gives on the fp32 cache holding the same (widened) values
    w = f16.to(torch.float32)
    assert w.dtype == torch.float32 and torch.equal(w.vn, f16.vn.float()) and torch.equal(w.vprime, f16.vprime.float())
    y16, att16 = m.answer(f16, qd, qld, BANK_INDEX, return_attention=True)
    y32, att32 = m.answer(w, qd, qld, BANK_INDEX, return_attention=True)
    assert torch.equal(y16, y32) and torch.equal(att16, att32) and float(y32.abs().max()) > 0
    p16, p32 = m.predict(f16, qd, qld, BANK_INDEX, k=3), m.predict(w, qd, qld, BANK_INDEX, k=3)
    assert torch.equal(p16.indices, p32.indices) and torch.equal(p16.probs, p32.probs)
    qf = m.encode_questions(qd[:3], qld[:3])
    qidx = torch.tensor([0, 1, 2, 0, 1, 2, 1])
    z16, z32 = m.answer_pairs(f16, qf, BANK_INDEX, qidx), m.answer_pairs(w, qf, BANK_INDEX, qidx)
    assert torch.equal(z16, z32) and float(z32.abs().max()) > 0
    pp16, pp32 = m.predict_pairs(f16, qf, BANK_INDEX, qidx, k=2), m.predict_pairs(w, qf, BANK_INDEX, qidx, k=2)
    assert torch.equal(pp16.indices, pp32.indices) and torch.equal(pp16.probs, pp32.probs)
    # a train-mode step on the cache: row 0 unasked, repeats (BANK_INDEX); the same seed draw for both
    m.train()
    steps = []
    for feats in (f16, w):
        torch.manual_seed(123)
        steps.append(features_step(m, feats, q, ql, a_idx, a_val, BANK_INDEX))
    assert m._last_ctx.p_att == 0.3 and m._last_ctx.seed != 0
    _same_step(*steps)
    assert not torch.equal(steps[0][0], y16)                           # the dropout masks did something
    # a vn-only float16 bank built in two chunks trains like the one-chunk bank
    one = _encode(m, v, with_vprime=False, dtype=torch.float16)
    two = ImageFeatures.cat([_encode(m, v[:1], with_vprime=False, dtype=torch.float16),
                             _encode(m, v[1:], with_vprime=False, dtype=torch.float16)])
    assert one.vprime is None and two.vprime is None and two.dtype == torch.float16 and two.N == v.shape[0]
    assert torch.equal(_bits(two.vn), _bits(one.vn)) and torch.equal(_bits(one.vn), _bits(f16.vn))
    bank_steps = []
    for feats in (one, two):
        torch.manual_seed(123)
        bank_steps.append(features_step(m, feats, q, ql, a_idx, a_val, BANK_INDEX))
    _same_step(*bank_steps)
    _same_step(bank_steps[0], steps[0])
    with pytest.raises(ValueError, match="storage formats"):
        ImageFeatures.cat([one, _encode(m, v[1:], with_vprime=False)])
    with pytest.raises(ValueError, match="torch.float32 or torch.float16"):
        _encode(m, v, dtype=torch.bfloat16)


# ----------------------------------------------------------------------------- how far a float16 cache is from the fp32 cache
# Measured on an MI355X (profiles/half_features_parity.txt): max |logit(float16 cache) - logit(fp32 cache)| on the 224 x 224
# fixture.  The run is deterministic; the factor 4 below only has to absorb a later change of summation order upstream of
# the cache.
RECORDED_LOGIT_DIFF = {"fp32": 1.862645e-07, "fp32x3": 1.927838e-07}


def measure_full224(compute_dtype):
    """answer() from a float16 cache against answer() from the fp32 cache (the parent's code path) on the 224 x 224 fixture:
    (max abs logit difference, max abs attention difference, fraction of questions whose top-1 changes, questions)."""
    meta, cfg, batch, image_index = _full224_case()
    v, q, ql, _, _ = batch
    torch.manual_seed(meta["seed"])
    m = build(cfg, meta["V"], compute_dtype=compute_dtype).eval()
    f32 = m.encode_images(v.to(DEV))
    f16 = m.encode_images(v.to(DEV), dtype=torch.float16)
    y32, a32 = m.answer(f32, q.to(DEV), ql.to(DEV), image_index, return_attention=True)
    y16, a16 = m.answer(f16, q.to(DEV), ql.to(DEV), image_index, return_attention=True)
    torch.cuda.synchronize()
    flips = float((y16.argmax(1) != y32.argmax(1)).float().mean())
    return (float((y16 - y32).abs().max()), float((a16 - a32).abs().max()), flips, q.shape[0], float(y32.abs().max()),
            float(a32.max()))


@pytest.mark.parametrize("compute_dtype", ["fp32", "fp32x3"])
def test_half_cache_answers_differ_from_fp32_cache_by_the_rounding_only(compute_dtype):
    d_logit, d_att, flips, n_q, y_max, a_max = measure_full224(compute_dtype)
    print(f"[half] full224 {compute_dtype}: max |dlogit| {d_logit:.3e} (largest |logit| {y_max:.3e}), max |datt| {d_att:.3e} "
          f"(largest weight {a_max:.3e}), top-1 changed for {flips * n_q:.0f} of {n_q} questions")
    assert d_logit > 0                                                  # the cache really is 16-bit
    assert d_logit < 4 * RECORDED_LOGIT_DIFF[compute_dtype]


if __name__ == "__main__":
    for dt in ("fp32", "fp32x3"):
        d_logit, d_att, flips, n_q, y_max, a_max = measure_full224(dt)
        print(f"full224 fixture, compute_dtype {dt}, {n_q} questions on 2 images, answer(float16 cache) vs answer(fp32 cache):")
        print(f"  max abs logit difference      {d_logit:.6e}   (largest |logit| {y_max:.6e})")
        print(f"  max abs attention difference  {d_att:.6e}   (largest attention weight {a_max:.6e})")
        print(f"  top-1 answer changed          {flips * n_q:.0f} of {n_q} questions ({flips:.3f})")
