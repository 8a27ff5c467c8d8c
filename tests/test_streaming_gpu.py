"""GPU parity of the streaming (HBM-bound) kernels of csrc/elementwise.hip and the units split from it (att_apply.hip,
gather.hip, adam.hip) against float64, in every mode, at the tails and past the grid cap.

The references are tests/streaming_ref.py (float64, CPU).  Every dropout mask is data from keep_scale -- the numpy
restatement of the counter-based hash -- never the output of a kernel, so the element index a fused kernel uses is
pinned here and not only through the whole model.  Output buffers are pre-filled with NaN (or a sentinel where pad
columns must survive), which shows unwritten elements and out-of-range writes alike.

Tolerances: the reference is float64, so the whole error is the kernel's.  A result that is a sum of n fp32 terms
gets max|err| / max|ref| <= 4 * 2^-24 * sqrt(n) (tol_sum); where tests/test_kernels_gpu.py already holds the same
kernel to a looser bound that one is used (3e-6 scores and probabilities, 1e-5 attention backward, 2e-5 two chained
reductions).  Masking, copies and single fp32 operations are compared for equality.  A bf16 output may differ by one
bf16 rounding of the fp32 value: |got - ref| <= 2^-8 |ref| + T max|ref|, for every element, with T = 1e-6 or, in the
L2-norm section, the fp32 tolerance of the same case.
"""
import math

import numpy as np
import pytest
import torch

from tests import streaming_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CAP_N = 8192 * 256          # threads of a capped element-wise grid: one more element and the grid-stride loop strides
SEED = 0x5EED0BAD1DEA0042    # both 32-bit words of the seed take part in the hash
NAN = float("nan")


def _ops():
    from dl_vqa_amd import ops
    return ops


def _raw(name, *args):
    """An entry point called directly, for the outputs that dl_vqa_amd.ops allocates itself (torch.empty): the tests
    hand in NaN-filled buffers instead."""
    from dl_vqa_amd import _lib
    _lib.call(name, *[a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args], _lib.stream())


def check(name, got, ref, tol):
    e = R.rel_err(got, ref)
    print(f"[parity] {name}: max|err|/max|ref| = {e:.3e} (tol {tol:.1e})")
    assert bool(torch.isfinite(got).all()), f"{name}: unwritten / non-finite elements"
    assert e <= tol, f"{name}: {e} > {tol}"


def check_bf16(name, got, ref, T=1e-6):
    """one bf16 rounding of the fp32 value on top of its own error T (relative to max|ref|), element-wise, no element exempt"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert bool(torch.isfinite(got).all()), f"{name}: unwritten / non-finite elements"
    bound = 2.0 ** -8 * ref.abs() + T * float(ref.abs().max())
    excess = float(((got - ref).abs() - bound).max())
    worst = float(((got - ref).abs() / bound.clamp_min(1e-300)).max())
    print(f"[parity] {name}: max |err| / (2^-8 |ref| + {T:.1e} max|ref|) = {worst:.3e} (tol 1)")
    assert excess <= 0.0, f"{name}: an element is {excess} outside one bf16 rounding"


def tol_sum(n, floor=0.0):
    return max(4 * 2.0 ** -24 * math.sqrt(n), floor)


def dev(t, dtype=None):
    return None if t is None else (t if dtype is None else t.to(dtype)).contiguous().to(DEV)


def nan_like(*shape, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype, device=DEV)


# ----------------------------------------------------------------------------- a. dropout against the restatement
@pytest.fixture(scope="module")
def cap_masks():
    """keep-scales of the first CAP_N + 3 elements, computed once on the CPU"""
    n = CAP_N + 3
    return {0.0: torch.from_numpy(R.keep_scale(SEED, n, 0.0)), 0.3: torch.from_numpy(R.keep_scale(SEED, n, 0.3))}


@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("inplace", [False, True])
def test_dropout_is_the_restated_hash(cap_masks, p, inplace):
    """n = 8192*256 + 3: the last three elements are reached only by the second trip of the grid-stride loop."""
    ops = _ops()
    n = CAP_N + 3
    x = torch.ones(n, device=DEV)
    y = x if inplace else nan_like(n)
    ops.dropout(x, p, SEED, out=y)
    torch.cuda.synchronize()
    want = cap_masks[p]
    assert torch.equal(y.cpu(), want), f"{int((y.cpu() != want).sum())} elements differ; first at " \
                                       f"{int((y.cpu() != want).nonzero()[0])}"
    if p > 0:
        assert 0.69 < float((want > 0).float().mean()) < 0.71


@pytest.mark.parametrize("p", [0.0, 0.3])
def test_dropout_add_and_dropout_to_bf16(cap_masks, p):
    ops = _ops()
    n = CAP_N + 3
    g = torch.Generator().manual_seed(11)
    x, acc = torch.randn(n, generator=g), torch.randn(n, generator=g)
    mask = cap_masks[p]
    y = acc.clone().to(DEV)
    ops.dropout_add(x.to(DEV), y, p, SEED)
    yb = torch.full((n,), NAN, dtype=torch.bfloat16, device=DEV)
    _raw("vqa_dropout_to_bf16", x.to(DEV), yb, n, p, SEED)
    torch.cuda.synchronize()
    # x * mask is one fp32 rounding (exact for a dropped element); the add is one more, or none if the compiler
    # contracted the pair into a fused multiply-add: |err| <= 2^-24 (|x * mask| + |acc + x * mask|) either way
    prod = x.double() * mask.double()
    want = acc.double() + prod
    err = (y.cpu().double() - want).abs()
    bound = 2.0 ** -24 * (prod.abs() + want.abs()) * (1 + 1e-6)
    print(f"[parity] dropout_add p={p}: max err/bound = {float((err / bound.clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= bound).all())
    dropped = mask == 0
    assert torch.equal(y.cpu()[dropped], acc[dropped])                       # a dropped element adds exactly nothing
    assert torch.equal(yb.cpu(), (x * mask).to(torch.bfloat16))               # fp32 product, round to nearest even


# ----------------------------------------------------------------------------- b. att_score_bwd
BWD_SHAPES = [(2, 9, 24, 2),          # one split, P % 4 = 1
              (3, 130, 1028, 1),      # RS = 2, rows_per = 65 (prefetch tail of 1), 257 column chunks > 256 threads
              (1, 257, 256, 4),       # RS = 3, rows_per = 86, G = 4
              (2, 1100, 64, 3)]       # RS at its cap of 8, a short last split, G = 3


def _score_bwd_inputs(B, P, mid, G, mode, p):
    g = torch.Generator().manual_seed(B * 1000 + P + mid + 7 * mode)
    xld = 2 * mid if mode == 2 else mid
    vp = torch.randn(B * P, mid, generator=g)
    qp = torch.randn(B, mid, generator=g)                 # both signs: the '|' ReLU on q' matters
    wx, bx = torch.randn(G, xld, generator=g), torch.randn(G, generator=g)
    ds = torch.randn(B, G, P, generator=g)
    mask = R.mask_tensor(SEED + mode, (B * P, xld), p)
    return vp, qp, wx, bx, ds, mask


@pytest.mark.parametrize("B,P,mid,G", BWD_SHAPES)
@pytest.mark.parametrize("xdtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_att_score_bwd(mode, p, xdtype, B, P, mid, G):
    """vqa_att_score_bwd in the three modes, with and without dropout, on fp32 and on bf16 x rewritten in place.
    fp32 x: float64 autograd through relu(v' op q') from v' and q'.  bf16 x: the closed form with the stored bf16 x as
    the ReLU's value (equal to the autograd form for an unrounded x, tests/test_streaming_ref_cpu.py)."""
    ops = _ops()
    from dl_vqa_amd import _lib
    vp, qp, wx, bx, ds, mask = _score_bwd_inputs(B, P, mid, G, mode, p)
    xld = wx.shape[1]
    x = R.att_x(vp, qp, mode, B, P).to(xdtype)           # fp32 arithmetic on the CPU: what the GEMM epilogue stores
    assert 0.4 < float((x == 0).float().mean()) < 0.6
    if xdtype == torch.float32:
        dv, dq, dwx, _ = R.att_score_bwd_ref(vp, qp, wx, bx, mask, mode, B, P, ds)
    else:
        dv, dq, dwx, _ = R.att_score_bwd_closed(x, vp, qp, wx, mask, mode, B, P, ds)
    RS = _lib.load().vqa_att_row_splits(P)
    assert RS == min(8, (P + 127) // 128)
    xs = x.clone().to(DEV)
    dwx_part, dq_part = nan_like(B * RS, G * xld), nan_like(B * RS, mid)
    _raw("vqa_att_score_bwd", dev(ds), dev(wx), xld, xs, int(xdtype == torch.bfloat16), dwx_part, dq_part, B, P, mid, G,
         p, SEED + mode, mode, dev(vp) if mode == 1 else None, dev(qp) if mode != 0 else None)
    dq_got, dwx_got = nan_like(B, mid), nan_like(G * xld)
    ops.sum_parts(dq_part, dq_got, B, RS, mid)
    ops.colsum(dwx_part, B * RS, G * xld, dwx_got)
    torch.cuda.synchronize()
    tag = f"att_score_bwd mode={mode} p={p} {'bf16' if xdtype == torch.bfloat16 else 'fp32'} {B, P, mid, G}"
    assert bool(torch.isfinite(dwx_part).all()) and bool(torch.isfinite(dq_part).all()), "a part was left unwritten"
    if xdtype == torch.float32:
        check(f"{tag} dv'", xs, dv, 1e-5)
    else:
        check_bf16(f"{tag} dv'", xs, dv)
    check(f"{tag} dq'", dq_got, dq, tol_sum(P, 1e-5))
    dwx_got = dwx_got.view(G, xld)
    check(f"{tag} dwx (v' half)", dwx_got[:, :mid], dwx[:, :mid], tol_sum(B * P, 1e-5))
    if mode == 2:
        check(f"{tag} dwx (q' half)", dwx_got[:, mid:], dwx[:, mid:], tol_sum(B * P, 1e-5))


# ----------------------------------------------------------------------------- c. att_score_fwd, every device path
FWD_CASES = [
    # (path, B, P, mid, G, bf16, qcat)
    ("general-fp32", 3, 37, 1028, 3, False, False),
    ("general-fp32", 3, 37, 1280, 1, False, False),     # a multiple of 256, but above 1024
    ("general-fp32", 3, 37, 24, 4, False, False),
    ("general-fp32-qcat", 3, 37, 24, 1, False, True),
    ("general-fp32-qcat", 3, 37, 24, 2, False, True),
    ("general-fp32-qcat", 3, 37, 256, 1, False, True),
    ("general-fp32-qcat", 3, 37, 256, 2, False, True),
    ("rows-bf16", 3, 37, 8, 1, True, False), ("rows-bf16", 3, 37, 8, 4, True, False),
    ("rows-bf16", 3, 37, 72, 1, True, False), ("rows-bf16", 3, 37, 72, 4, True, False),
    ("rows-bf16", 3, 37, 520, 1, True, False), ("rows-bf16", 3, 37, 520, 4, True, False),
    ("rows-bf16", 3, 37, 1024, 1, True, False), ("rows-bf16", 3, 37, 1024, 4, True, False),
    ("general-bf16", 3, 37, 1032, 2, True, False),
    ("general-bf16", 3, 37, 12, 3, True, False),
    ("general-bf16-qcat", 3, 37, 64, 2, True, True),
    # past the grid cap of 8192 blocks x 4 waves: the m += nwaves trip, and the nxt / cur hand-over across it
    ("rows-fp32-wrap", 49, 676, 256, 2, False, False),      # 33 124 rows > 32 768 waves
    ("general-fp32-wrap", 49, 676, 24, 2, False, False),
    ("rows-bf16-wrap", 97, 676, 64, 2, True, False),        # 65 572 rows > 2 x 32 768
]


@pytest.mark.parametrize("path,B,P,mid,G,bf16,qcat", FWD_CASES,
                         ids=[f"{c[0]}-{c[1]}x{c[2]}-mid{c[3]}-G{c[4]}" for c in FWD_CASES])
@pytest.mark.parametrize("p", [0.0, 0.3])
def test_att_score_fwd(p, path, B, P, mid, G, bf16, qcat):
    """The four device paths of vqa_att_score_fwd (fp32 rows kernel, general fp32, bf16 rows kernel, general bf16),
    with and without the concatenated q' half, against float64 from the stored x."""
    g = torch.Generator().manual_seed(B + P + mid + G)
    M = B * P
    assert M % 2 == 1 or "wrap" in path
    mode = 2 if qcat else 0
    xld = 2 * mid if qcat else mid
    x = torch.relu(torch.randn(M, mid, generator=g)).to(torch.bfloat16 if bf16 else torch.float32)
    qp = torch.randn(B, mid, generator=g)
    wx, bx = torch.randn(G, xld, generator=g), torch.randn(G, generator=g)
    mask = R.mask_tensor(SEED, (M, xld), p)
    want = R.att_score_from_x(x.double(), qp.double(), wx.double(), bx.double(),
                              None if mask is None else mask.double(), mode, B, P)
    score = nan_like(B, G, P)
    _raw("vqa_att_score_fwd", dev(x), int(bf16), dev(wx), xld, dev(bx), score, B, P, mid, G, p, SEED,
         dev(qp) if qcat else None)
    torch.cuda.synchronize()
    check(f"att_score_fwd {path} {B, P, mid, G} p={p}", score, want, tol_sum(xld, 3e-6))


# ----------------------------------------------------------------------------- d. att_apply_bwd
def _peaked(score):
    """Scores scaled by 30, then the runner-up of every row placed 3 below its maximum and everything else at least 12
    below: one probability near 1 (0.95), one at 0.05, the rest small down to an underflow to 0.  The gap is fixed
    because d score of a row is O(runner-up probability) while the fp32 rounding of s = sum_p probs * dprob enters the
    top element at 2^-24 |dprob| whatever the gap: with the runner-up left to chance max|dscore| of a single-row case
    can be 1e-6 |dprob| and the relative figure then measures the conditioning of the softmax Jacobian, not the
    kernel."""
    s = score * 30
    top2 = s.topk(2, dim=-1)
    top = top2.values[..., :1]
    s = torch.minimum(s, top - 12.0)
    s.scatter_(-1, top2.indices[..., :1], top)
    s.scatter_(-1, top2.indices[..., 1:], top - 3.0)
    return s


@pytest.mark.parametrize("B,P,C,G", [(2, 300, 72, 3), (1, 65, 520, 1), (3, 17, 64, 4), (49, 676, 8, 2)])
@pytest.mark.parametrize("peaked", [False, True], ids=["ordinary", "peaked"])
def test_att_apply_bwd(peaked, B, P, C, G):
    """Both kernels of vqa_att_apply_bwd against float64 autograd through softmax + weighted sum: P > 256 (the block
    loop of softmax_bwd), C/4 > 64 (lane loop with a tail), rows past the grid cap, peaked probabilities, the
    rowsum output, and want_dvn=False."""
    g = torch.Generator().manual_seed(B * 100 + P + C + G)
    score = torch.randn(B, G, P, generator=g) * 2
    if peaked:
        score = _peaked(score)
    vn = torch.randn(B, P, C, generator=g)
    ld = G * C + 12
    dout = torch.randn(B, ld, generator=g)
    pr, dscore_ref, dvn_ref = R.att_apply_bwd_ref(score, vn, dout[:, :G * C])
    if peaked:
        assert float(pr.max(-1).values.min()) > 0.9 and float(pr.min()) < 2.0 ** -149      # one near 1, some 0 in fp32
    probs = dev(pr, torch.float32)
    dscore, dvn, rowsum = nan_like(B, G, P), nan_like(B, P, C), nan_like(B, G)
    _raw("vqa_att_apply_bwd", dev(dout), ld, probs, dev(vn), dscore, dvn, rowsum, B, P, C, G)
    dscore2 = nan_like(B, G, P)
    _raw("vqa_att_apply_bwd", dev(dout), ld, probs, dev(vn), dscore2, None, None, B, P, C, G)
    torch.cuda.synchronize()
    tag = f"att_apply_bwd {'peaked' if peaked else 'ordinary'} {B, P, C, G}"
    check(f"{tag} dscore", dscore, dscore_ref, 1e-5)
    check(f"{tag} dvn", dvn, dvn_ref, 1e-5)
    assert torch.equal(dscore, dscore2), "want_dvn=False changed dscore"
    # the true row sum is 0 (softmax is shift invariant), so the kernel's sum is held to the float64 sum of its OWN
    # dscore: P additions of values up to max|dscore|, each rounded to fp32
    own = dscore.double().sum(-1).cpu()
    bound = P * 2.0 ** -23 * float(dscore.abs().max())
    err = float((rowsum.double().cpu() - own).abs().max())
    print(f"[parity] {tag} rowsum: max|err| = {err:.3e} (bound {bound:.3e})")
    assert bool(torch.isfinite(rowsum).all()) and err <= bound


# ----------------------------------------------------------------------------- e. att_apply_fwd at the edges of softmax
@pytest.mark.parametrize("B,P,C,G,kind", [(2, 40, 20, 2, "offset"), (3, 1, 24, 3, "one"), (2, 5, 72, 2, "five")])
def test_att_apply_fwd_softmax_edges(B, P, C, G, kind):
    g = torch.Generator().manual_seed(P + C)
    score = torch.randn(B, G, P, generator=g)
    if kind == "offset":      # exp overflows without the max subtraction; fp32 scores near 1e4, taken as they are
        score = (1e4 + (torch.rand(B, G, P, generator=g) * 180 - 90)).float()
    vn = torch.randn(B, P, C, generator=g)
    pr, ref = R.att_apply_ref(score, vn)
    ld = G * C + 4
    out = torch.full((B, ld), 7.0, device=DEV)
    probs = nan_like(B, G, P)
    _raw("vqa_att_apply_fwd", dev(score), dev(vn), probs, out, ld, B, P, C, G)
    torch.cuda.synchronize()
    assert bool((out[:, G * C:] == 7.0).all())
    if kind == "one":         # a single position: probability exactly 1, the output exactly that row of vn
        assert bool((probs == 1.0).all())
        assert torch.equal(out[:, :G * C].cpu(), vn[:, 0, :].repeat(1, G))
        return
    check(f"att_apply_fwd {kind} probs {B, P, C, G}", probs, pr, 3e-6)
    check(f"att_apply_fwd {kind} out {B, P, C, G}", out[:, :G * C], ref, 3e-6)


# ----------------------------------------------------------------------------- f. softce
def _softce_case(A):
    """Five rows, each one adversity; no row repeats an answer index; a_val is non-zero on the ignored entries."""
    g = torch.Generator().manual_seed(A)
    B, K = 5, 10
    logits = torch.randn(B, A, generator=g) * 3
    a_idx = torch.zeros(B, K, dtype=torch.int64)
    a_val = torch.randint(1, 8, (B, K), generator=g)
    nv = min(K, A)

    def answers(b, first=()):
        rest = [i for i in (torch.randperm(A, generator=g) + 1).tolist() if i not in first]
        ids = list(first) + rest
        a_idx[b, :nv] = torch.tensor(ids[:nv])
    # row 0: the maximum at two indices that different waves serve (thread = index % 256, wave = thread / 64; A = 3
    # has one wave only): the score follows the FIRST, whose count (4 -> 1.0) differs from the second's (1 -> 0.3)
    i1, i2 = {3: (0, 2), 257: (5, 200)}.get(A, (5, 700))
    logits[0, i1] = logits[0, i2] = float(logits[0].max()) + 1.5
    answers(0, (i2 + 1, i1 + 1))
    a_val[0, 0], a_val[0, 1] = 1, 4
    # row 1: all logits equal -> arg-max 0
    logits[1] = 0.5
    answers(1, (1,))
    a_val[1, 0] = 2
    # row 2: logits near +-1e4
    logits[2] = torch.randn(A, generator=g) + 1e4 * (torch.randint(0, 2, (A,), generator=g) * 2 - 1)
    answers(2)
    # row 3: padding entries and an entry above A around valid ones
    answers(3)
    a_idx[3, 0] = 0
    a_idx[3, nv - 1] = A + 1
    if nv > 3:
        a_idx[3, 2] = 0
    # row 4: no valid answer at all
    a_idx[4] = 0
    a_idx[4, 3] = A + 7
    for b in range(B):
        v = a_idx[b][(a_idx[b] > 0) & (a_idx[b] <= A)]
        assert len(set(v.tolist())) == len(v)
    return logits, a_idx, a_val


@pytest.mark.parametrize("A", [3, 257, 1000, 3000])
def test_softce_adverse_rows(A):
    """vqa_softce_fwd_bwd against the oracle in float64, row by row (a row near 1e4 must not set the scale for the
    others).  A = 3, row 2 is the regression case of the loss arithmetic: with every logit near +1e4 the kernel's
    former (max + log(sum)) - logit rounded the log-sum-exp at 1e4 (half an ulp = 5e-4) against a loss term of order 1
    and missed the 3e-6 bound at 1.3e-4; log(sum) - (logit - max) has no such cancellation."""
    logits, a_idx, a_val = _softce_case(A)
    B = logits.shape[0]
    loss_ref, score_ref, dl_ref = R.soft_ce_ref(logits, a_idx, a_val)
    assert float(score_ref[0]) == 1.0 and abs(float(score_ref[1]) - 0.6) < 1e-6 and float(loss_ref[4]) == 0.0
    ld = A + 4
    lg = nan_like(B, ld)
    lg[:, :A] = logits.to(DEV)                                   # NaN in the pad columns: a read of one poisons the row
    dl = torch.full((B, ld), 7.0, device=DEV)
    loss, score = nan_like(B), nan_like(B)
    _raw("vqa_softce_fwd_bwd", lg, ld, dev(a_idx), dev(a_val), a_idx.shape[1], B, A, 1.0 / B, loss, score, dl, ld)
    loss2, score2 = nan_like(B), nan_like(B)
    _raw("vqa_softce_fwd_bwd", lg, ld, dev(a_idx), dev(a_val), a_idx.shape[1], B, A, 1.0 / B, loss2, score2, None, 0)
    torch.cuda.synchronize()
    assert bool((dl[:, A:] == 7.0).all()), "dlogits pad columns were written"
    assert torch.equal(loss, loss2) and torch.equal(score, score2), "dlogits=None changed loss / score"
    names = ["two maxima", "all equal", "near +-1e4", "padding and > A", "no valid answer"]
    for b in range(B):
        if b == 4:
            assert float(loss[b]) == 0.0 and float(score[b]) == 0.0 and float(dl[b, :A].abs().max()) == 0.0
            continue
        check(f"softce A={A} row {b} ({names[b]}) loss", loss[b], loss_ref[b], 3e-6)
        check(f"softce A={A} row {b} ({names[b]}) dlogits", dl[b, :A], dl_ref[b], tol_sum(A, 1e-5))
    check(f"softce A={A} score rows", score, score_ref, 1e-6)


# ----------------------------------------------------------------------------- g. fused dropout against float64
@pytest.mark.parametrize("binned", [True, False], ids=["binned", "scanning"])
def test_embed_tanh_with_dropout(binned):
    ops = _ops()
    V, E, B, T = 40, 12, 9, 5
    p = 0.3
    g = torch.Generator().manual_seed(21)
    emb = torch.randn(V, E, generator=g)
    q = torch.randint(0, V, (B, T), generator=g)
    q[0, 1] = 0
    q[3, 2] = q[5, 4] = q[7, 0] = 6                       # one row gathers several slots
    dx = torch.randn(T, B, E, generator=g)
    mask = R.mask_tensor(SEED, (B, T, E), p)
    x_ref, demb_ref = R.embed_tanh_ref(q, emb, mask, dx)
    x = nan_like(T, B, E)
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    _raw("vqa_embed_tanh_fwd", dev(q), dev(emb), x, B, T, E, V, p, SEED, bad)
    demb = nan_like(V, E)
    # backward from the float64 forward rounded to fp32: the test of the backward does not lean on the forward kernel
    ops.embed_tanh_bwd(dev(q), dev(x_ref, torch.float32), dev(dx), demb, p, SEED, binned=binned)
    torch.cuda.synchronize()
    check("embed_tanh_fwd p=0.3", x, x_ref, 2e-6)
    check(f"embed_tanh_bwd p=0.3 {'binned' if binned else 'scanning'}", demb, demb_ref, 5e-6)
    assert int(bad) == 0 and float(demb[0].abs().max()) == 0.0


@pytest.mark.parametrize("rows,C,bwd", [(37, 32, True), (37, 288, True),
                                        (32771, 8, False),        # more rows than the capped grid has waves
                                        (4 * 32768 + 3, 8, False),  # four rows per wave: the register form strides here
                                        (32771, 260, False)])     # the two-pass form strides here
def test_l2norm_with_input_dropout(rows, C, bwd):
    ops = _ops()
    p = 0.3
    g = torch.Generator().manual_seed(rows + C)
    u = torch.randn(rows, C, generator=g)
    mask = R.mask_tensor(SEED, (rows, C), p)
    dv = torch.randn(rows, C, generator=g) if bwd else None
    ref = R.l2norm_ref(u, mask, dv)
    vn, norm = nan_like(rows, C), nan_like(rows)
    _raw("vqa_l2norm_fwd", dev(u), vn, norm, rows, C, p, SEED, None, 0, 0.0, 0)
    torch.cuda.synchronize()
    check(f"l2norm_fwd p=0.3 vn {rows, C}", vn, ref[0], 2e-6)
    check(f"l2norm_fwd p=0.3 norm {rows, C}", norm, ref[1], 2e-6)
    if bwd:
        # from the float64 forward rounded to fp32, as above
        du = nan_like(rows, C)
        ops.l2norm_bwd(dev(dv), dev(ref[0], torch.float32), dev(ref[1], torch.float32), p, SEED, out=du)
        torch.cuda.synchronize()
        check(f"l2norm_bwd p=0.3 {rows, C}", du, ref[2], 5e-6)


@pytest.mark.parametrize("p", [0.0, 0.3])
def test_relu_drop_bwd_in_place_past_the_cap(cap_masks, p):
    ops = _ops()
    n = CAP_N + 3
    g = torch.Generator().manual_seed(5)
    y = torch.relu(torch.randn(n, generator=g))
    y[torch.arange(0, n, 7)] = 0.0
    y[torch.arange(3, n, 11)] = -0.0                       # +0.0 and -0.0 pass no gradient
    y[n - 1], y[n - 2] = 2.0, 0.0
    dy = torch.randn(n, generator=g)
    want = dy * (y > 0) * cap_masks[p]                     # one fp32 product: exact
    d = dy.clone().to(DEV)
    ops.relu_drop_bwd(y.to(DEV), d, d, p, SEED)            # in place on dy, as the engine calls it
    torch.cuda.synchronize()
    assert torch.equal(d.cpu(), want), f"{int((d.cpu() != want).sum())} elements differ"


# ----------------------------------------------------------------------------- h. helpers
def test_scale_by_past_the_cap():
    ops = _ops()
    n = CAP_N + 1
    g = torch.Generator().manual_seed(1)
    x = torch.randn(n, generator=g)
    k = torch.tensor([0.37], dtype=torch.float32)
    xd = x.clone().to(DEV)
    ops.scale_by(xd, k.to(DEV))
    torch.cuda.synchronize()
    assert torch.equal(xd.cpu(), x * k)


@pytest.mark.parametrize("with_b", [True, False])
@pytest.mark.parametrize("inplace", [False, True])
def test_add2d_strided(with_b, inplace):
    ops = _ops()
    rows, cols, lda, ldb, ldy = 37, 50, 64, 52, 56
    g = torch.Generator().manual_seed(2)
    a, b = torch.randn(rows, lda, generator=g), torch.randn(rows, ldb, generator=g)
    want = a[:, :cols] + (b[:, :cols] if with_b else 0.0)
    ad, bd = a.clone().to(DEV), b.to(DEV)
    y = ad if inplace else torch.full((rows, ldy), 7.0, device=DEV)
    ops.add2d(ad, lda, bd if with_b else None, ldb, y, lda if inplace else ldy, rows, cols)
    torch.cuda.synchronize()
    assert torch.equal(y[:, :cols].cpu(), want)
    if inplace:
        assert torch.equal(y[:, cols:].cpu(), a[:, cols:])         # pad columns untouched
    else:
        assert bool((y[:, cols:] == 7.0).all())


def test_adam_with_gradient_scale_past_the_cap():
    ops = _ops()
    n = CAP_N + 5
    g = torch.Generator().manual_seed(3)
    p, gr = torch.randn(n, generator=g), torch.randn(n, generator=g) * 3
    m, v = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    pr = p.double()
    pd, gd = p.clone().to(DEV), gr.to(DEV)
    md, vd = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    for step in (1, 2, 3):
        lr = 5e-4 * 0.5 ** ((step - 1) / 50000)
        R.adam_ref(pr, gr.double(), m, v, step, lr, 0.37)
        ops.adam(pd, gd, md, vd, lr, step, grad_scale=0.37)
    torch.cuda.synchronize()
    check("adam grad_scale=0.37 p", pd, pr, 1e-6)
    check("adam grad_scale=0.37 m", md, m, tol_sum(2 * 3))     # three steps of beta1 * m + (1 - beta1) * g
    check("adam grad_scale=0.37 v", vd, v, tol_sum(2 * 3))
    tail = slice(n - 5, n)                                       # the elements only the second trip reaches
    check("adam tail p", pd[tail], pr[tail], 1e-6)
    check("adam tail v", vd[tail], v[tail], tol_sum(2 * 3))


@pytest.mark.parametrize("rows,cols,ld", [(256, 1, 1), (40, 70, 70), (100000, 3, 3), (1000, 70, 76)])
def test_colsum_shapes(rows, cols, ld):
    ops = _ops()
    g = torch.Generator().manual_seed(rows + cols)
    x = torch.randn(rows, ld, generator=g)
    x[:, cols:] = NAN                                            # pad columns must not be read
    out = nan_like(cols)
    ops.colsum(x.to(DEV), rows, cols, out, ld=ld)
    torch.cuda.synchronize()
    check(f"colsum {rows, cols} ld={ld}", out, x[:, :cols].double().sum(0), tol_sum(rows, 1e-5))


def test_colsum_masked_accumulate():
    ops = _ops()
    rows, cols = 5000, 130
    g = torch.Generator().manual_seed(10)
    x = torch.randn(rows, cols, generator=g)
    mask = torch.randint(0, 5, (rows, cols), generator=g).to(torch.uint8)
    init = torch.randn(cols, generator=g)
    out = init.clone().to(DEV)
    ops.colsum(x.to(DEV), rows, cols, out, mask=mask.to(DEV), accumulate=True)
    torch.cuda.synchronize()
    check("colsum masked+acc (5000, 130)", out, (x.double() * (mask != 4)).sum(0) + init.double(), tol_sum(rows, 1e-5))


@pytest.mark.parametrize("B,G,P", [(1, 2, 1), (17, 3, 65), (40, 1, 676)])
def test_sum_bgp_shapes(B, G, P):
    ops = _ops()
    g = torch.Generator().manual_seed(B + P)
    x = torch.randn(B, G, P, generator=g) + 0.5
    out = nan_like(G)
    ops.sum_bgp(x.to(DEV), out)
    torch.cuda.synchronize()
    check(f"sum_bgp {B, G, P}", out, x.double().sum((0, 2)), tol_sum(B * P))


@pytest.mark.parametrize("batch,parts,cols", [(3, 1, 257), (2, 8, 1024)])
def test_sum_parts_shapes(batch, parts, cols):
    ops = _ops()
    g = torch.Generator().manual_seed(parts + cols)
    part = torch.randn(batch * parts, cols, generator=g)
    out = nan_like(batch, cols)
    ops.sum_parts(part.to(DEV), out, batch, parts, cols)
    torch.cuda.synchronize()
    check(f"sum_parts {batch, parts, cols}", out, part.double().reshape(batch, parts, cols).sum(1), tol_sum(parts))


# ----------------------------------------------------------------------------- i. L2 norm: every output mode against float64
SEED_V = 0xC0FFEE1234ABCDEF   # the dropout in front of the image projection; SEED is the image dropout
GUARD = 64                    # NaN elements before and after every output
INV_EPS32 = float(np.float32(1.0) / np.float32(1e-12))          # 1 / (0 + 1e-12) as the kernels evaluate it

L2_SHAPES = [
    # (B, Hp, Wp, C, G, bf16 row-major output too, a pooled row of zeros)
    (3, 5, 7, 16, 1, True, True),      # four active lanes; row pairs that straddle an image; 105 rows: the last pair clamps
    (3, 5, 7, 48, 3, True, True),      # three channel blocks: c >> 2 and c & 3 both vary
    (2, 3, 3, 256, 4, True, False),    # every lane active
    (2, 3, 3, 272, 2, True, False),    # the two-pass form with a second trip of 4 lanes; 17 blocks
    (1, 7, 5, 512, 4, True, False),
    (97, 26, 26, 16, 2, False, False),     # 65 572 rows > 2 x 32 768 waves: the register form strides
    (49, 26, 26, 272, 1, False, False),    # 33 124 rows > 32 768 waves: the two-pass form strides
]


def _guarded(n, dtype):
    """a NaN buffer of n elements between two NaN guards: (flat, the view to hand to the kernel)"""
    flat = torch.full((n + 2 * GUARD,), NAN, dtype=dtype, device=DEV)
    return flat, flat[GUARD:GUARD + n]


def _guards_intact(name, flat, n):
    ints = flat.view(torch.int32 if flat.dtype == torch.float32 else torch.int16)
    want = torch.full((1,), NAN, dtype=flat.dtype).view(ints.dtype).item()
    assert bool((ints[:GUARD] == want).all()) and bool((ints[GUARD + n:] == want).all()), f"{name}: a guard element was written"


def _l2_judge(name, got, ref, ref_zero, zero_row, T, bf16):
    """every row but the all-zero one against the float64 gradient in the max norm of those rows; the all-zero row on its
    own, relative to its own maximum, against dvn * (1 / (0 + 1e-12)) with the quotient evaluated in fp32"""
    got = got.detach().double().cpu()
    assert bool(torch.isfinite(got).all()), f"{name}: unwritten / non-finite elements"
    keep = torch.ones(got.shape[0], dtype=torch.bool)
    parts = [(name, got, ref)]
    if zero_row is not None:
        keep[zero_row] = False
        parts = [(name, got[keep], ref[keep]), (name + " all-zero row", got[zero_row], ref_zero)]
    for n, a, b in parts:
        if bf16:
            check_bf16(n, a, b, T)
        else:
            check(n, a, b, T)


@pytest.mark.parametrize("B,Hp,Wp,C,G,rowmajor_bf16,zero", L2_SHAPES, ids=[f"{s[0]}x{s[1]}x{s[2]}-C{s[3]}-G{s[4]}" for s in L2_SHAPES])
@pytest.mark.parametrize("p_v,p", [(0.0, 0.0), (0.3, 0.3)])
def test_l2norm_bwd_every_output_mode(p_v, p, B, Hp, Wp, C, G, rowmajor_bf16, zero):
    """vqa_l2norm_bwd and vqa_l2norm_bwd_joined with the fp32, the bf16 and the channel-blocked bf16 output against float64:
    dvn = sum_g probs * dout + mask_v * dv_in (tests/streaming_ref.py; for the plain entry point that sum rounded to fp32 is
    the input), pushed through autograd of u / (|u| + 1e-12), u = mask * pooled.  Masks are R.mask_tensor's; vn and norm are
    the float64 forward rounded to fp32.  fp32: 5e-6 of max|ref| (plain), + tol_sum(G + 1) for the join's G + 1-term sum;
    bf16: |got - ref| <= 2^-8 |ref| + T max|ref| for every element, T the fp32 tolerance.  Outputs lie between NaN guards,
    dout has NaN pad columns, the channel-blocked output is un-blocked with tests/conv_lattice_ref.py's from_c16."""
    from tests.conv_lattice_ref import from_c16
    P = Hp * Wp
    rows = B * P
    g = torch.Generator().manual_seed(rows * 7 + C + G)
    pooled = torch.randn(rows, C, generator=g)
    zero_row = P + 1 if zero else None
    if zero:
        pooled[zero_row] = 0.0
    probs = torch.softmax(torch.randn(B, G, P, generator=g) * 2, dim=-1)
    ld = G * C + 8
    dout = torch.full((B, ld), NAN)
    dout[:, :G * C] = torch.randn(B, G * C, generator=g)
    dv_in = torch.randn(rows, C, generator=g)
    mask, mask_v = R.mask_tensor(SEED, (rows, C), p), R.mask_tensor(SEED_V, (rows, C), p_v)
    vn, norm = R.l2norm_ref(pooled, mask)
    assert not zero or (float(norm[zero_row]) == 0.0 and float(vn[zero_row].abs().max()) == 0.0)
    dvn = R.l2norm_join_ref(probs, dout[:, :G * C], dv_in, mask_v)
    dvn32 = dvn.to(torch.float32)
    m1 = 1.0 if mask is None else mask.double()
    refs = {"joined": (R.l2norm_ref(pooled, mask, dvn)[2], dvn, 5e-6 + tol_sum(G + 1)),
            "plain": (R.l2norm_ref(pooled, mask, dvn32)[2], dvn32.double(), 5e-6)}
    vn_d, norm_d, dout_d, probs_d, dv_in_d, dvn_d = dev(vn, torch.float32), dev(norm, torch.float32), dev(dout), dev(probs), dev(dv_in), dev(dvn32)
    modes = [(0, "fp32"), (2, "c16")] + ([(1, "bf16")] if rowmajor_bf16 else [])
    for entry, (ref, a, T) in refs.items():
        ref_zero = None if not zero else (a * INV_EPS32 * m1)[zero_row]
        for mode, mname in modes:
            flat, out = _guarded(rows * C, torch.float32 if mode == 0 else torch.bfloat16)
            if entry == "joined":
                _raw("vqa_l2norm_bwd_joined", dout_d, ld, probs_d, G, dv_in_d, p_v, SEED_V, vn_d, norm_d, out, mode, rows, P, C, p, SEED)
            else:
                _raw("vqa_l2norm_bwd", dvn_d, vn_d, norm_d, out, mode, rows, P, C, p, SEED)
            torch.cuda.synchronize()
            name = f"l2norm_bwd {entry} {mname} {B, Hp, Wp, C, G} p_v={p_v} p={p}"
            _guards_intact(name, flat, rows * C)
            got = out.view(rows, C) if mode != 2 else from_c16(out.view(B, C // 16, Hp, Wp, 16)).reshape(rows, C)
            _l2_judge(name, got, ref, ref_zero, zero_row, T, mode != 0)
    assert bool(torch.isnan(dout_d[:, G * C:]).all())


@pytest.mark.parametrize("rows,C", [(37, 272), (4 * 32768 + 3, 8)])
@pytest.mark.parametrize("p2", [0.3, 0.0])
def test_l2norm_fwd_second_output(p2, rows, C):
    """vqa_l2norm_fwd's second output vdrop = dropout_{p2}(vn), fp32 and bf16, in the two-pass form and in the register form past
    the grid cap, against float64 mask2 * vn; p2 = 0 copies vn.  fp32: 2e-6, the bound vn is held to; bf16: one rounding on top."""
    p = 0.3
    g = torch.Generator().manual_seed(rows + C + 1)
    u = torch.randn(rows, C, generator=g)
    mask, mask2 = R.mask_tensor(SEED, (rows, C), p), R.mask_tensor(SEED_V, (rows, C), p2)
    vn_ref, norm_ref = R.l2norm_ref(u, mask)
    want = vn_ref if mask2 is None else vn_ref * mask2.double()
    ud = dev(u)
    for dtype, is_bf16 in ((torch.float32, 0), (torch.bfloat16, 1)):
        vn, norm = nan_like(rows, C), nan_like(rows)
        flat, vd = _guarded(rows * C, dtype)
        _raw("vqa_l2norm_fwd", ud, vn, norm, rows, C, p, SEED, vd, is_bf16, p2, SEED_V)
        torch.cuda.synchronize()
        name = f"l2norm_fwd vdrop {'bf16' if is_bf16 else 'fp32'} {rows, C} p2={p2}"
        _guards_intact(name, flat, rows * C)
        check(f"{name}: vn", vn, vn_ref, 2e-6)
        check(f"{name}: norm", norm, norm_ref, 2e-6)
        if is_bf16:
            check_bf16(name, vd.view(rows, C), want, 2e-6)
        else:
            check(name, vd.view(rows, C), want, 2e-6)
        if p2 > 0:
            dropped = (mask2 == 0)
            assert 0.25 < float(dropped.float().mean()) < 0.35 and bool((vd.view(rows, C).cpu()[dropped] == 0).all())
