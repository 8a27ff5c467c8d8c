"""float64 references for the deletion and insertion curves of VqaNet.explain_faithfulness / explain_faithfulness_pairs
(include/vqa_hip.h vqa_rank_desc, vqa_occl_curves):

  rank_desc            the positions of every row by descending value under the header's total order;
  kept_sets            the kept set of every step of both curves, as masks;
  brute_curves         attribution_ref.forward64 on a per-question bank with the absent rows zeroed: 2 (P + 1) forwards;
  kernel_form_curves   the kept form from the operands the entry point takes (base, U, probs, score, cnull, order, ...);
  closed_curves        the same from a state dict: v', q', cnull, U and base by their products, then kernel_form_curves;
  sequential_curves    the kernel's own order of sums (chunks of L steps, prefixes and suffixes over chunks, the walk) restated
                       with torch on the host in a chosen dtype: what fp32 loses along 676 sequential adds.

Everything here runs on the CPU; the GPU tests import it and compute each reference once."""
import functools

import torch

from tests import attribution_ref as R


def rank_desc(maps):
    """order int64 [B, P]: larger value first, equal values by the smaller position, -0.0 equal to +0.0, every NaN behind
    -inf (several by position)."""
    v = torch.as_tensor(maps).detach().float().cpu().reshape(len(maps), -1)
    nan = torch.isnan(v)
    v = torch.where(nan, torch.full_like(v, float("-inf")), v).double()
    # a stable descending sort puts equal values (and -0.0 beside +0.0) in ascending position; then the NaNs go last, stably
    first = torch.sort(v, dim=1, descending=True, stable=True).indices
    last = torch.sort(nan.gather(1, first).to(torch.int8), dim=1, stable=True).indices
    return first.gather(1, last)


def kept_sets(order, P):
    """(deletion, insertion) masks [B, P+1, P] (float64): mask[b, k, s] = 1 where position s is PRESENT at step k.  An order
    entry outside [0, P) names no position."""
    order = torch.as_tensor(order, dtype=torch.int64)
    B = order.shape[0]
    valid = (order >= 0) & (order < P)
    onehot = torch.zeros(B, P, P, dtype=torch.float64)                  # [b, step, position]
    onehot.scatter_(2, order.clamp(0, P - 1)[..., None], valid.double()[..., None])
    first = torch.cat([torch.zeros(B, 1, P, dtype=torch.float64), onehot.cumsum(1)], 1)      # the first k steps' positions
    return first[:, -1:, :] - first, first


def brute_curves(sd, do_option, vn, qf, img, answers, grid, order):
    """(deletion, insertion) [B, P+1] in float64: the logit of features with the absent rows zeroed.  order must be a
    permutation per row."""
    img = torch.as_tensor(img, dtype=torch.int64)
    cols = torch.as_tensor(answers, dtype=torch.int64)[:, None]
    B, P = len(img), vn.shape[1]
    one = torch.arange(B)
    bank = vn.double()[img]                 # question b reads row b of a bank of its own
    out = []
    for mask in kept_sets(order, P):
        curve = torch.empty(B, P + 1, dtype=torch.float64)
        for k in range(P + 1):
            curve[:, k] = R.forward64(sd, do_option, bank * mask[:, k, :, None], qf, one, grid).gather(1, cols)[:, 0]
        out.append(curve)
    return tuple(out)


def kernel_form_curves(base, U, slot, probs, score, cnull, W2, b2, answers, order):
    """What vqa_occl_curves computes, in float64.  base [B, hid], U [R, P, G, hid], slot [B], probs and score [B, G, P], cnull
    [B, G], W2 [A, hid], b2 [A], answers [B], order [B, P] (|K| counts steps, an entry outside [0, P) adds nothing).  Returns a
    dict: deletion, insertion [B, P+1], alpha_del, alpha_ins [B, G, P+1], r [B, G]."""
    base, U, probs, score, cnull, W2, b2 = (x.double() for x in (base, U, probs, score, cnull, W2, b2))
    slot, answers = torch.as_tensor(slot, dtype=torch.int64), torch.as_tensor(answers, dtype=torch.int64)
    B, G, P = probs.shape
    m = score.max(-1, keepdim=True).values
    r = (torch.exp(cnull.reshape(m.shape) - m) / torch.exp(score - m).sum(-1, keepdim=True))[..., 0]
    steps = torch.arange(P + 1, dtype=torch.float64)
    out = {"r": r}
    for name, mask, absent in zip(("deletion", "insertion"), kept_sets(order, P), (steps, P - steps)):
        mass = torch.einsum("bks,bgs->bgk", mask, probs)
        alpha = 1.0 / (mass + absent[None, None, :] * r[..., None])
        acc = torch.einsum("bks,bgs,bsgh->bgkh", mask, probs, U[slot])
        pre = base[:, None, :] + (alpha[..., None] * acc).sum(1)
        out[name] = torch.einsum("bkh,bh->bk", torch.relu(pre), W2[answers]) + b2[answers][:, None]
        out["alpha_" + name[:3]] = alpha
    return out


def closed_curves(sd, do_option, vn, qf, img, answers, grid, order):
    """(deletion, insertion) [B, P+1] by the kept form, in float64, from a state dict, and kernel_form_curves' dict."""
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
    hid = w1.shape[0]
    U = torch.einsum("hgc,npc->npgh", w1[:, :G * C].reshape(hid, G, C), vn)
    base = b1 + qf @ w1[:, G * C:].t()
    parts = kernel_form_curves(base, U, img, probs, score, cnull, sd["classifier.lin2.weight"], sd["classifier.lin2.bias"], cols,
                               order)
    return parts["deletion"], parts["insertion"], parts


def sequential_curves(base, U, slot, probs, score, cnull, W2, b2, answers, order, L, dtype):
    """The curves by the kernel's order of sums, in `dtype` on the host: chunk sums of L steps from 0 in ascending order,
    exclusive prefixes over the chunks ascending and suffixes descending, then each chunk's rows added one by one -- forward from
    the prefix (insertion), backward from the suffix (deletion).  order: a permutation per row.  r and the final dot product
    are formed by torch in `dtype` (their lengths are vqa_occl_logit's).  Returns (deletion, insertion) [B, P+1]."""
    base, U, probs, score, cnull, W2, b2 = (x.to(dtype) for x in (base, U, probs, score, cnull, W2, b2))
    slot, answers = torch.as_tensor(slot, dtype=torch.int64), torch.as_tensor(answers, dtype=torch.int64)
    order = torch.as_tensor(order, dtype=torch.int64)
    B, G, P = probs.shape
    m = score.max(-1, keepdim=True).values
    r = (torch.exp(cnull.reshape(m.shape) - m) / torch.exp(score - m).sum(-1, keepdim=True))[..., 0]         # [B, G]
    one = torch.arange(B)
    w = probs.gather(2, order[:, None, :].expand(B, G, P))                                                  # [B, G, step]
    rows = w[..., None] * U[slot][one[:, None], order].permute(0, 2, 1, 3)                                  # [B, G, step, hid]
    zero_h, zero_m = torch.zeros_like(rows[:, :, 0]), torch.zeros_like(w[:, :, 0])
    nch = (P + L - 1) // L
    sums, masses = [], []
    for c in range(nch):
        s, ms = zero_h.clone(), zero_m.clone()
        for k in range(c * L, min(P, (c + 1) * L)):
            s, ms = s + rows[:, :, k], ms + w[:, :, k]
        sums.append(s), masses.append(ms)
    pre, suf = [None] * nch, [None] * nch
    run, run_m = zero_h.clone(), zero_m.clone()
    for c in range(nch):
        pre[c] = (run, run_m)
        run, run_m = run + sums[c], run_m + masses[c]
    run, run_m = zero_h.clone(), zero_m.clone()
    for c in reversed(range(nch)):
        suf[c] = (run, run_m)
        run, run_m = run + sums[c], run_m + masses[c]
    w2, bias = W2[answers], b2[answers]

    def logit(acc, mass, absent):
        alpha = 1.0 / (mass + absent * r)
        return (torch.relu(base + (alpha[..., None] * acc).sum(1)) * w2).sum(-1) + bias

    deletion = torch.empty(B, P + 1, dtype=dtype)
    insertion = torch.empty(B, P + 1, dtype=dtype)
    for c in range(nch):
        k0, k1 = c * L, min(P, (c + 1) * L)
        acc, mass = pre[c]
        if c == 0:
            insertion[:, 0] = logit(acc, mass, P)
        for k in range(k0, k1):
            acc, mass = acc + rows[:, :, k], mass + w[:, :, k]
            insertion[:, k + 1] = logit(acc, mass, P - (k + 1))
        acc, mass = suf[c]
        if c == nch - 1:
            deletion[:, P] = logit(acc, mass, P)
        for k in reversed(range(k0, k1)):
            acc, mass = acc + rows[:, :, k], mass + w[:, :, k]
            deletion[:, k] = logit(acc, mass, k)
    return deletion, insertion


@functools.lru_cache(maxsize=None)
def _fixture_brute_curves(do_option, answers, order):
    f = R.fixture_case(do_option)
    return brute_curves(f["golden"].sd, do_option, f["vn"], f["qf"], f["img"], list(answers), f["grid"], torch.tensor(order))


def fixture_brute_curves(do_option, answers, order):
    """brute_curves of the fixture's pairs (attribution_ref.fixture_case) for the given answer columns and ranking, computed
    once per (fixture, columns, ranking) and shared by the tests that need it."""
    order = torch.as_tensor(order).tolist()
    return _fixture_brute_curves(do_option, tuple(int(a) for a in answers), tuple(tuple(int(s) for s in row) for row in order))
