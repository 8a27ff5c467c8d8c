"""The float64 references of tests/streaming_ref.py stand on their own (no GPU, no HIP library) before they judge a
kernel: the numpy restatement of the dropout hash behaves like a dropout mask, the closed-form attention-score
backward equals the autograd form, and the soft-target cross entropy equals log_softmax arithmetic."""
import math

import numpy as np
import pytest
import torch

from tests import streaming_ref as R


@pytest.mark.parametrize("p", [0.1, 0.3, 0.5])
def test_keep_scale_rate_and_value(p):
    n = 1 << 20
    m = R.keep_scale(0x1234567811223344, n, p)
    assert m.dtype == np.float32 and m.shape == (n,)
    vals = np.unique(m)
    inv_keep = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    assert vals.tolist() == [0.0, float(inv_keep)]
    # the drop probability is floor(p * 65536) / 65536: p to within 2^-16, far inside the binomial bound
    keep = float((m > 0).mean())
    assert abs(keep - (1 - p)) <= 4 * math.sqrt(p * (1 - p) / n), keep


def test_keep_scale_p0_seeds_and_index_form():
    assert np.array_equal(R.keep_scale(77, 1000, 0.0), np.ones(1000, dtype=np.float32))
    a, b = R.keep_scale(77, 4096, 0.3), R.keep_scale(78, 4096, 0.3)
    assert not np.array_equal(a, b)
    assert not np.array_equal(a, R.keep_scale(77 + (1 << 32), 4096, 0.3))      # the high seed word takes part
    assert np.array_equal(a, R.keep_scale(77, 4096, 0.3))
    # the mask is a pure function of (seed, element index): a slice equals the indexed form
    idx = np.array([5, 4095, 0, 17, 2, 3], dtype=np.uint64)
    assert np.array_equal(R.keep_scale_at(77, idx, 0.3), a[idx.astype(np.int64)])
    # an element pair shares one hash (low / high 16 bits): both halves are used, and they differ
    even, odd = a[0::2] > 0, a[1::2] > 0
    assert 0.2 < float((even != odd).mean()) < 0.6


def test_keep_scale_known_hash():
    """mix32 / drop_hash restated by hand in Python integers for a few (seed, index) pairs."""
    def mix(x):
        x ^= x >> 16; x = (x * 0x7FEB352D) & 0xFFFFFFFF; x ^= x >> 15; x = (x * 0x846CA68B) & 0xFFFFFFFF; x ^= x >> 16
        return x
    p = 0.3
    thr = int(np.uint32(np.float32(p) * np.float32(65536.0)))
    assert thr == 19660
    for seed in (0, 991, 0xDEADBEEF12345678):
        for i in (0, 1, 2, 7, 1000001, (1 << 33) + 5):
            pair = i >> 1
            h = mix((pair & 0xFFFFFFFF) ^ (seed & 0xFFFFFFFF))
            h = mix((h + (pair >> 32) * 0x9E3779B9 + (seed >> 32)) & 0xFFFFFFFF)
            u = (h >> 16) if i & 1 else (h & 0xFFFF)
            got = float(R.keep_scale_at(seed, [i], p)[0])
            assert (got > 0) == (u >= thr), (seed, i)


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("p", [0.0, 0.3])
def test_closed_form_score_backward_equals_autograd(mode, p):
    B, P, mid, G = 3, 11, 20, 3
    g = torch.Generator().manual_seed(40 + mode)
    xld = 2 * mid if mode == 2 else mid
    vp = torch.randn(B * P, mid, generator=g, dtype=torch.float64)
    qp = torch.randn(B, mid, generator=g, dtype=torch.float64)
    wx = torch.randn(G, xld, generator=g, dtype=torch.float64)
    bx = torch.randn(G, generator=g, dtype=torch.float64)
    ds = torch.randn(B, G, P, generator=g, dtype=torch.float64)
    mask = R.mask_tensor(5150, (B * P, xld), p)
    want = R.att_score_bwd_ref(vp, qp, wx, bx, mask, mode, B, P, ds)
    x = R.att_x(vp, qp, mode, B, P)
    assert 0.3 < float((x == 0).double().mean()) < 0.7
    got = R.att_score_bwd_closed(x, vp, qp, wx, mask, mode, B, P, ds)
    for name, a, b in zip(("dv'", "dq'", "dwx", "dbx"), got, want):
        assert R.rel_err(a, b) <= 1e-12, (name, R.rel_err(a, b))
    # and the forward from the stored x is the forward of the block
    assert R.rel_err(R.att_score_from_x(x, qp, wx, bx, mask.double() if mask is not None else None, mode, B, P),
                     R.att_score_ref(vp, qp, wx, bx, mask, mode, B, P)) <= 1e-12


def test_score_reference_is_the_oracle_attention_block():
    """att_score_ref restates oracle.attention_scores after its two projections (identity projections here)."""
    from oracle import vqa_oracle as O
    B, g_, mid, G = 2, 3, 8, 2
    P = g_ * g_
    gen = torch.Generator().manual_seed(3)
    v = torch.randn(B, mid, g_, g_, generator=gen, dtype=torch.float64)
    q = torch.randn(B, mid, generator=gen, dtype=torch.float64)
    for mode, opt in enumerate("+*|"):
        xld = 2 * mid if mode == 2 else mid
        wx = torch.randn(G, xld, generator=gen, dtype=torch.float64)
        bx = torch.randn(G, generator=gen, dtype=torch.float64)
        mask = R.mask_tensor(9, (B * P, xld), 0.3).double()
        sd = {"attention.v_conv.weight": torch.eye(mid, dtype=torch.float64)[:, :, None, None],
              "attention.q_lin.weight": torch.eye(mid, dtype=torch.float64),
              "attention.q_lin.bias": torch.zeros(mid, dtype=torch.float64),
              "attention.x_conv.weight": wx[:, :, None, None], "attention.x_conv.bias": bx}
        masks = {"att_x": mask.reshape(B, g_, g_, xld).permute(0, 3, 1, 2)}
        want = O.attention_scores(sd, v, q, opt, masks).reshape(B, G, P)
        vp = v.permute(0, 2, 3, 1).reshape(B * P, mid)
        assert R.rel_err(R.att_score_ref(vp, q, wx, bx, mask, mode, B, P), want) <= 1e-12


def test_soft_ce_reference_is_log_softmax_arithmetic():
    g = torch.Generator().manual_seed(6)
    B, A, K = 6, 37, 4
    logits = torch.randn(B, A, generator=g) * 3
    a_idx = torch.zeros(B, K, dtype=torch.int64)
    a_val = torch.randint(1, 8, (B, K), generator=g)
    for b in range(B):
        k = 1 + b % K
        a_idx[b, :k] = torch.randperm(A, generator=g)[:k] + 1
    a_idx[1, 3] = A + 2                                       # ignored, like the padding index
    a_idx[2, 0] = int(logits[2].argmax()) + 1
    rows, score, dl = R.soft_ce_ref(logits, a_idx, a_val)
    ls = torch.log_softmax(logits.double(), dim=1)
    sm = torch.softmax(logits.double(), dim=1)
    for b in range(B):
        want, grad, agree = 0.0, torch.zeros(A, dtype=torch.float64), 0
        for k in range(K):
            i = int(a_idx[b, k])
            if i == 0 or i > A:
                continue
            w = float(a_val[b, k]) / 10.0
            want -= w * float(ls[b, i - 1])
            grad += w * sm[b]
            grad[i - 1] -= w
            if i - 1 == int(logits[b].argmax()):
                agree = int(a_val[b, k])
        assert abs(float(rows[b]) - want / B) <= 1e-12 * max(1.0, abs(want))
        assert float((dl[b] - grad / B).abs().max()) <= 1e-14
        assert abs(float(score[b]) - min(1.0, 0.3 * agree)) <= 1e-6
    assert float(score[2]) > 0


def test_adam_reference_scales_the_gradient():
    from oracle import vqa_oracle as O
    g = torch.Generator().manual_seed(2)
    p, gr = torch.randn(50, generator=g, dtype=torch.float64), torch.randn(50, generator=g, dtype=torch.float64)
    m, v = torch.zeros(50, dtype=torch.float64), torch.zeros(50, dtype=torch.float64)
    p2, m2, v2 = p.clone(), m.clone(), v.clone()
    R.adam_ref(p, gr, m, v, 1, 1e-3, 0.5)
    f = lambda s: float(np.float32(s))
    O.adam_step(p2, gr * 0.5, m2, v2, 1, f(1e-3), f(0.9), f(0.999), f(1e-8))
    assert torch.equal(p, p2) and torch.equal(m, m2) and torch.equal(v, v2)


@pytest.mark.parametrize("p_v,p", [(0.0, 0.0), (0.3, 0.3)])
def test_l2norm_join_closed_form_equals_autograd_through_the_stage(p_v, p):
    """The gradient vqa_l2norm_bwd_joined joins in closed form (weighted-sum branch + dropout branch), pushed through the
    normalisation, is autograd through softmax-weighted sum + dropout + normalise."""
    B, P, C, G = 2, 5, 8, 3
    g = torch.Generator().manual_seed(3)
    pooled = torch.randn(B * P, C, generator=g).double()
    score = torch.randn(B, G, P, generator=g).double()
    dout = torch.randn(B, G * C, generator=g).double()
    dv_in = torch.randn(B * P, C, generator=g).double()
    mask = R.mask_tensor(0x1122334455667788, (B * P, C), p)
    mask_v = R.mask_tensor(0x8877665544332211, (B * P, C), p_v)
    probs, want = R.l2norm_join_autograd(pooled, mask, score, dout, dv_in, mask_v)
    dvn = R.l2norm_join_ref(probs, dout, dv_in, mask_v)
    got = R.l2norm_ref(pooled, mask, dvn)[2]
    assert R.rel_err(got, want) < 1e-13
    # the two branches are both there: either alone is a different gradient
    for part in (R.l2norm_join_ref(probs, dout, torch.zeros_like(dv_in), mask_v), R.l2norm_join_ref(torch.zeros_like(probs), dout, dv_in, mask_v)):
        assert R.rel_err(R.l2norm_ref(pooled, mask, part)[2], want) > 1e-2
    if p > 0:
        assert float((mask == 0).float().mean()) > 0.1 and bool((got[mask == 0] == 0).all())


def test_l2norm_all_zero_row_in_float64():
    """A pooled row of zeros: vn = 0, norm = 0, and the gradient is dvn / 1e-12 -- what the kernels are held to on that row."""
    g = torch.Generator().manual_seed(4)
    pooled = torch.randn(3, 8, generator=g).double()
    pooled[1] = 0
    dvn = torch.randn(3, 8, generator=g).double()
    vn, nrm, d = R.l2norm_ref(pooled, None, dvn)
    assert float(vn[1].abs().max()) == 0 and float(nrm[1]) == 0
    assert R.rel_err(d[1], dvn[1] * 1e12) < 1e-12
