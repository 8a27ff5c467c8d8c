"""Float64 CPU references for the streaming (HBM-bound) kernels of csrc/elementwise.hip and the units split from it
(att_apply.hip, gather.hip, adam.hip).

Nothing here touches the GPU or the HIP library: the dropout masks are recomputed from the counter-based hash of
csrc/common.hpp in numpy (keep_scale), every operator is plain float64 torch, and the attention-score backward exists
twice -- through autograd and in closed form -- so that one form checks the other (tests/test_streaming_ref_cpu.py)
before either judges a kernel (tests/test_streaming_gpu.py).

Layouts are the kernels': x / v' / masks are [B*P, channels] with row m = b*P + p, scores and probabilities are
[B, G, P], q' is [B, mid], wx is [G, xld] with xld = mid ('+', '*') or 2*mid ('|').  mode 0 '+', 1 '*', 2 '|'.
"""
import numpy as np
import torch

from oracle import vqa_oracle as O

_M32 = np.uint64(0xFFFFFFFF)


def _mix32(x):
    """mix32 of csrc/common.hpp on uint64 arrays holding 32-bit values."""
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & _M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & _M32
    x = x ^ (x >> np.uint64(16))
    return x


def keep_scale_at(seed: int, idx, p: float) -> np.ndarray:
    """drop_scale(seed, idx, p, 1/(1-p)) of csrc/common.hpp for an array of flat element indices: one 32-bit hash per
    PAIR of elements (idx >> 1), the even element takes its low 16 bits and the odd one the high 16; an element is
    kept iff its field is at or above uint32(p * 65536.0f).  Returns 0 or 1/(1-p) as float32."""
    idx = np.asarray(idx, dtype=np.uint64)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    s_lo, s_hi = np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)
    pair = idx >> np.uint64(1)
    lo, hi = pair & _M32, pair >> np.uint64(32)
    h = _mix32(lo ^ s_lo)
    h = _mix32((h + ((hi * np.uint64(0x9E3779B9)) & _M32) + s_hi) & _M32)
    u = np.where((idx & np.uint64(1)) == 1, h >> np.uint64(16), h & np.uint64(0xFFFF))
    pf = np.float32(p)
    thr = np.uint64(np.uint32(pf * np.float32(65536.0)))
    inv_keep = np.float32(1.0) / (np.float32(1.0) - pf) if p > 0 else np.float32(1.0)
    return np.where(u >= thr, inv_keep, np.float32(0.0)).astype(np.float32)


def keep_scale(seed: int, n: int, p: float) -> np.ndarray:
    """The keep-scale (0 or 1/(1-p), float32) of elements 0..n-1 of a dropout site with this seed."""
    return keep_scale_at(seed, np.arange(n, dtype=np.uint64), p)


def mask_tensor(seed: int, shape, p: float):
    """keep_scale over a logical row-major tensor of this shape as a float32 torch tensor; None when p == 0."""
    if p <= 0:
        return None
    n = int(np.prod(shape))
    return torch.from_numpy(keep_scale(seed, n, p)).reshape(*shape)


def rel_err(got: torch.Tensor, ref: torch.Tensor) -> float:
    got = got.detach().double().cpu()
    ref = ref.detach().double().cpu()
    scale = max(float(ref.abs().max()), 1e-30)
    return float((got - ref).abs().max()) / scale


# ----------------------------------------------------------------------------- attention score
def _d(t):
    return None if t is None else t.detach().double()


def att_x(vprime, qp, mode: int, B: int, P: int):
    """The v' half of x: relu(v' + tile(q')), relu(v' * tile(q')) or relu(v') -- [B*P, mid], in the dtype given."""
    qt = qp.repeat_interleave(P, dim=0)
    if mode == 0:
        return torch.relu(vprime + qt)
    if mode == 1:
        return torch.relu(vprime * qt)
    return torch.relu(vprime)


def _x_full(x, qp, mode: int, P: int):
    """x over all xld channels: for '|' the q' half relu(tile(q')) is appended."""
    if mode != 2:
        return x
    return torch.cat([x, torch.relu(qp).repeat_interleave(P, dim=0)], dim=1)


def att_score_from_x(x, qp, wx, bx, mask, mode: int, B: int, P: int):
    """score[b,g,p] = bx[g] + sum_n (mask * x)[b*P+p, n] * wx[g, n] from the ReLU output x [B*P, mid] (for '|' the q'
    half comes from qp); mask over the logical [B*P, xld] tensor, or None."""
    xf = _x_full(x, qp, mode, P)
    if mask is not None:
        xf = xf * mask
    return (xf @ wx.t() + bx).reshape(B, P, -1).permute(0, 2, 1)


def att_score_ref(vprime, qp, wx, bx, mask, mode: int, B: int, P: int):
    """Float64 forward of the reference Attention block after the two projections: scores [B, G, P]."""
    vprime, qp, wx, bx, mask = _d(vprime), _d(qp), _d(wx), _d(bx), _d(mask)
    return att_score_from_x(att_x(vprime, qp, mode, B, P), qp, wx, bx, mask, mode, B, P)


def att_score_bwd_ref(vprime, qp, wx, bx, mask, mode: int, B: int, P: int, dscore):
    """Autograd backward of sum(score * dscore): (dv' [B*P, mid], dq' [B, mid], dwx [G, xld], dbx [G]), float64."""
    v = _d(vprime).requires_grad_(True)
    q = _d(qp).requires_grad_(True)
    w = _d(wx).requires_grad_(True)
    b = _d(bx).requires_grad_(True)
    score = att_score_from_x(att_x(v, q, mode, B, P), q, w, b, _d(mask), mode, B, P)
    (score * _d(dscore)).sum().backward()
    return v.grad, q.grad, w.grad, b.grad


def att_score_bwd_closed(x, vprime, qp, wx, mask, mode: int, B: int, P: int, dscore):
    """The same four gradients in closed form, with the STORED ReLU output x [B*P, mid] taken as the value of the
    ReLU: (x > 0) is the ReLU's derivative and x is what dwx sees.  This is the bf16 path's contract (x is kept as
    bf16, exact in float64); with x = att_x(v', q') unrounded it equals att_score_bwd_ref."""
    x, qp, wx, mask, dscore = _d(x), _d(qp), _d(wx), _d(mask), _d(dscore)
    mid = x.shape[1]
    G = wx.shape[0]
    ds = dscore.permute(0, 2, 1).reshape(B * P, G)             # [M, G]
    m1 = mask[:, :mid] if mask is not None else torch.ones_like(x)
    dz = (x > 0).double() * m1 * (ds @ wx[:, :mid])            # d loss / d (pre-ReLU v' half)
    dwx = torch.zeros_like(wx)
    dwx[:, :mid] = ds.t() @ (m1 * x)
    qt = qp.repeat_interleave(P, dim=0)
    if mode == 0:
        dv, dq = dz, dz.reshape(B, P, mid).sum(1)
    elif mode == 1:
        dv, dq = dz * qt, (dz * _d(vprime)).reshape(B, P, mid).sum(1)
    else:
        m2 = mask[:, mid:] if mask is not None else torch.ones_like(x)
        dv = dz
        dq = (qp > 0).double() * (m2 * (ds @ wx[:, mid:])).reshape(B, P, mid).sum(1)
        dwx[:, mid:] = ds.t() @ (m2 * torch.relu(qt))
    return dv, dq, dwx, ds.sum(0)


# ----------------------------------------------------------------------------- softmax + weighted sum
def att_apply_ref(score, vn):
    """probs [B,G,P] = softmax over positions, out [B, G*C] = sum_p probs * vn (glimpse-major), float64."""
    score, vn = _d(score), _d(vn)
    B, G, P = score.shape
    pr = torch.softmax(score, dim=-1)
    return pr, torch.einsum("bgp,bpc->bgc", pr, vn).reshape(B, -1)


def att_apply_bwd_ref(score, vn, dout):
    """Autograd backward of sum(out * dout): (probs, dscore [B,G,P], dvn [B,P,C]); dout [B, G*C]."""
    s = _d(score).requires_grad_(True)
    v = _d(vn).requires_grad_(True)
    B, G, P = s.shape
    pr = torch.softmax(s, dim=-1)
    out = torch.einsum("bgp,bpc->bgc", pr, v).reshape(B, -1)
    (out * _d(dout)).sum().backward()
    return pr.detach(), s.grad, v.grad


# ----------------------------------------------------------------------------- soft-target cross entropy
def soft_ce_ref(logits, a_idx, a_val):
    """Per-row loss (already divided by the batch size), VQA score per row and d loss / d logits, float64, from the
    oracle's soft_ce_loss / batch_accuracy.  Answer entries above A are ignored like the padding index 0 (the kernel
    skips them; the oracle's gather could not index them)."""
    B, A = logits.shape
    idx = torch.where(a_idx > A, torch.zeros_like(a_idx), a_idx)
    lg = _d(logits).requires_grad_(True)
    rows = torch.stack([O.soft_ce_loss(lg[b:b + 1], idx[b:b + 1], a_val[b:b + 1]) / B for b in range(B)])
    rows.sum().backward()
    score = torch.stack([O.batch_accuracy(lg[b:b + 1].detach(), idx[b:b + 1], a_val[b:b + 1]) for b in range(B)])
    return rows.detach(), score.double(), lg.grad


# ----------------------------------------------------------------------------- Adam with a gradient scale
def adam_ref(p, g, m, v, step: int, lr: float, grad_scale: float, beta1=0.9, beta2=0.999, eps=1e-8):
    """oracle.adam_step on grad * grad_scale, in place on float64 p, m, v.  The scalars are taken at the float32
    values the C ABI passes (the kernel never sees the double 0.999), so the whole difference is the kernel's."""
    f = lambda s: float(np.float32(s))
    O.adam_step(p, g * f(grad_scale), m, v, step, f(lr), f(beta1), f(beta2), f(eps))


# ----------------------------------------------------------------------------- L2 norm with input dropout
def l2norm_ref(pooled, mask, dvn=None):
    """vn = u / (|u| + 1e-12) with u = mask * pooled, per row; with dvn also d loss / d pooled.  Float64."""
    x = _d(pooled).requires_grad_(True)
    u = x if mask is None else x * _d(mask)
    nrm = u.norm(p=2, dim=1, keepdim=True)
    vn = u / (nrm.expand_as(u) + 1e-12)
    if dvn is None:
        return vn.detach(), nrm.detach()[:, 0]
    vn.backward(_d(dvn))
    return vn.detach(), nrm.detach()[:, 0], x.grad


def l2norm_join_ref(probs, dout, dv_in, mask_v):
    """d loss / d vn as vqa_l2norm_bwd_joined joins it: dvn[b*P+p] = sum_g probs[b,g,p] * dout[b, g*C:(g+1)*C] (the
    softmax-weighted sum's branch) + mask_v * dv_in (the branch through the dropout in front of the image projection).
    probs [B,G,P], dout [B, G*C], dv_in and mask_v [B*P, C] (mask_v None: no dropout).  Float64."""
    probs, dout, dv_in = _d(probs), _d(dout), _d(dv_in)
    B, G, P = probs.shape
    C = dv_in.shape[1]
    dvn = torch.einsum("bgp,bgc->bpc", probs, dout.reshape(B, G, C)).reshape(B * P, C)
    return dvn + (dv_in if mask_v is None else dv_in * _d(mask_v))


def l2norm_join_autograd(pooled, mask, score, dout, dv_in, mask_v):
    """d loss / d pooled by autograd through the whole stage: vn = normalise(mask * pooled), out = sum_p softmax(score) * vn,
    v_drop = mask_v * vn, loss = sum(out * dout) + sum(v_drop * dv_in).  Float64; returns (probs, d pooled)."""
    x = _d(pooled).requires_grad_(True)
    u = x if mask is None else x * _d(mask)
    vn = u / (u.norm(p=2, dim=1, keepdim=True) + 1e-12)
    B, G, P = score.shape
    pr = torch.softmax(_d(score), dim=-1)
    out = torch.einsum("bgp,bpc->bgc", pr, vn.reshape(B, P, -1)).reshape(B, -1)
    vd = vn if mask_v is None else vn * _d(mask_v)
    ((out * _d(dout)).sum() + (vd * _d(dv_in)).sum()).backward()
    return pr.detach(), x.grad


# ----------------------------------------------------------------------------- tanh(dropout(embedding))
def embed_tanh_ref(q, emb, mask, dx=None):
    """x [T, B, E] = tanh(mask[b, t, :] * emb[q[b, t]]), mask over the logical [B, T, E] tensor; row 0 is the padding
    index (no gradient).  With dx also d loss / d emb.  Float64."""
    e = _d(emb).requires_grad_(True)
    y = torch.nn.functional.embedding(q, e, padding_idx=0)       # [B, T, E]
    if mask is not None:
        y = y * _d(mask)
    x = torch.tanh(y).transpose(0, 1)
    if dx is None:
        return x.detach()
    x.backward(_d(dx))
    return x.detach(), e.grad
