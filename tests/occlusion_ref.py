"""float64 references for the occlusion maps of VqaNet.explain_occlusion / explain_occlusion_pairs (include/vqa_hip.h
vqa_occl_logit):

  windows        S(p) of every grid position: the window x window square centred on p, clipped at the border, as a mask [P, P];
  brute          logit - logit_occluded by attribution_ref.forward64 on vn with the rows of S(p) zeroed: P forwards per question;
  closed_form    the header's formulas restated from (vn, v', q', the weights, img, mode, window);
  kernel_form    the kernel's own part of them, from the operands the entry point takes (base, Z, U, probs, score, cnull, ...).

Everything here runs on the CPU; the GPU tests import it and compute each reference once."""
import functools

import torch

from tests import attribution_ref as R


def windows(gh, gw, window):
    """mask [P, P] (float64): mask[p, s] = 1 where s lies in S(p)."""
    assert window % 2 == 1
    h = window // 2
    ys, xs = torch.arange(gh).repeat_interleave(gw), torch.arange(gw).repeat(gh)
    near = ((ys[:, None] - ys[None, :]).abs() <= h) & ((xs[:, None] - xs[None, :]).abs() <= h)
    return near.double()


def brute(sd, do_option, vn, qf, img, answers, grid, window):
    """maps [B, P] in float64: the logit of the full features minus the logit of features with the rows of S(p) zeroed."""
    img = torch.as_tensor(img, dtype=torch.int64)
    cols = torch.as_tensor(answers, dtype=torch.int64)[:, None]
    B, P = len(img), vn.shape[1]
    mask = windows(*grid, window)
    one = torch.arange(B)
    full = R.forward64(sd, do_option, vn, qf, img, grid).gather(1, cols)[:, 0]
    maps = torch.empty(B, P, dtype=torch.float64)
    # question b reads row b of a bank of its own, so that questions about the same image do not share an occlusion
    bank = vn.double()[img]
    for p in range(P):
        occluded = bank * (1.0 - mask[p])[None, :, None]
        maps[:, p] = full - R.forward64(sd, do_option, occluded, qf, one, grid).gather(1, cols)[:, 0]
    return maps


def kernel_form(base, Z, U, slot, probs, score, cnull, W2, b2, answers, grid, window):
    """What vqa_occl_logit computes, in float64.  base [B, hid], Z [B, G, hid], U [R, P, G, hid], slot [B], probs and score
    [B, G, P], cnull [B, G], W2 [A, hid], b2 [A], answers [B].  Returns a dict: occluded (the occluded logit [B, P]), alpha
    and mass [B, G, P], r [B, G]."""
    base, Z, U, probs, score, cnull, W2, b2 = (x.double() for x in (base, Z, U, probs, score, cnull, W2, b2))
    slot, answers = torch.as_tensor(slot, dtype=torch.int64), torch.as_tensor(answers, dtype=torch.int64)
    mask = windows(*grid, window)                                       # [P, S]
    m = score.max(-1, keepdim=True).values
    r = (torch.exp(cnull.reshape(m.shape) - m) / torch.exp(score - m).sum(-1, keepdim=True))[..., 0]
    mass = torch.einsum("ps,bgs->bgp", mask, probs)
    alpha = 1.0 / (1.0 - mass + mask.sum(-1)[None, None, :] * r[..., None])
    taken = torch.einsum("ps,bgs,bsgh->bgph", mask, probs, U[slot])      # sum over S(p) of probs * U
    pre = base[:, None, :] + (alpha[..., None] * (Z[:, :, None, :] - taken)).sum(1)
    occluded = torch.einsum("bph,bh->bp", torch.relu(pre), W2[answers]) + b2[answers][:, None]
    return {"occluded": occluded, "alpha": alpha, "mass": mass, "r": r}


def closed_form(sd, do_option, vn, qf, img, answers, grid, window):
    """maps [B, P] by the closed form, in float64, from a state dict: v' and q' by their products, cnull as the header
    states it per do_option, then kernel_form.  Returns (maps, kernel_form's dict)."""
    sd = R._sd64(sd)
    img = torch.as_tensor(img, dtype=torch.int64)
    cols = torch.as_tensor(answers, dtype=torch.int64)
    vn, vp, qp, wx, bx, _dwv, _, mode = R.model_inputs(sd, do_option, vn, qf, img, cols)
    qf = qf.double()
    mid, (N, P, C), G = vp.shape[-1], vn.shape, wx.shape[0]
    score, _ = R.scores(vp, qp, wx, bx, img, mode)
    probs = torch.softmax(score, dim=-1)
    if mode == 0:
        cnull = torch.relu(qp) @ wx.t() + bx
    elif mode == 1:
        cnull = bx.expand(len(img), G)
    else:
        cnull = torch.relu(qp) @ wx[:, mid:].t() + bx
    w1, b1 = sd["classifier.lin1.weight"], sd["classifier.lin1.bias"]
    w2, b2 = sd["classifier.lin2.weight"], sd["classifier.lin2.bias"]
    hid = w1.shape[0]
    w1g = w1[:, :G * C].reshape(hid, G, C)
    U = torch.einsum("hgc,npc->npgh", w1g, vn)
    out = torch.einsum("bgp,bpc->bgc", probs, vn[img])
    Z = torch.einsum("hgc,bgc->bgh", w1g, out)
    base = b1 + qf @ w1[:, G * C:].t()
    parts = kernel_form(base, Z, U, img, probs, score, cnull, w2, b2, cols, grid, window)
    logit = (torch.relu(base + Z.sum(1)) @ w2.t() + b2).gather(1, cols[:, None])[:, 0]
    return logit[:, None] - parts["occluded"], parts


@functools.lru_cache(maxsize=None)
def _fixture_brute(do_option, answers, window):
    f = R.fixture_case(do_option)
    return brute(f["golden"].sd, do_option, f["vn"], f["qf"], f["img"], list(answers), f["grid"], window)


def fixture_brute(do_option, answers, window=1):
    """brute of the fixture's pairs (attribution_ref.fixture_case) for the given answer columns, computed once per (fixture,
    columns, window) and shared by the tests that need it."""
    return _fixture_brute(do_option, tuple(int(a) for a in answers), int(window))
