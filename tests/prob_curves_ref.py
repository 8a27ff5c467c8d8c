"""float64 references for the probability curves of VqaNet.explain_faithfulness_probs / explain_faithfulness_probs_pairs
(include/vqa_hip.h vqa_occl_curves_hidden, vqa_softmax_pick), built on tests/faithfulness_ref.py:

  brute_logit_curves   attribution_ref.forward64 on a per-question bank with the absent rows zeroed, every column kept:
                       logits [B, 2, P+1, A], deletion at [:, 0], insertion at [:, 1];
  curve_stats          softmax, the probability of a given column, the arg-max under the library's order (ties by the smaller
                       column), its probability and the margin between the best and the second logit, from such logits;
  brute_prob_curves    the two together;
  kernel_form_hidden   the kept form up to the hidden row, from the operands the entry point takes;
  closed_operands      those operands from a state dict (faithfulness_ref.closed_curves' products, kept);
  comparable           which (b, side, k) entries an fp32 arg-max may be compared at, and the share left out.

Everything here runs on the CPU; the GPU tests import it and compute each reference once."""
import functools

import torch

from tests import attribution_ref as R
from tests import faithfulness_ref as FR

MAX_LEFT_OUT = 0.05     # the largest share of (b, k) entries an arg-max comparison may leave out


def brute_logit_curves(sd, do_option, vn, qf, img, grid, order):
    """logits [B, 2, P+1, A] in float64 of features with the absent rows zeroed; order: a permutation per row."""
    img = torch.as_tensor(img, dtype=torch.int64)
    B, P = len(img), vn.shape[1]
    one = torch.arange(B)
    bank = vn.double()[img]                 # question b reads row b of a bank of its own
    sides = []
    for mask in FR.kept_sets(order, P):
        sides.append(torch.stack([R.forward64(sd, do_option, bank * mask[:, k, :, None], qf, one, grid) for k in range(P + 1)], 1))
    return torch.stack(sides, 1)


def curve_stats(logits, answers):
    """From logits [B, 2, K, A] (float64) and the columns [B]: a dict of prob [B, 2, K] (the softmax probability of the
    question's column; 0 for a column outside [0, A)), top int64 [B, 2, K] (the first maximum: ties by the smaller column),
    top_prob and margin [B, 2, K] (best minus second-best logit; inf for A == 1)."""
    logits = logits.double()
    B, _, K, A = logits.shape
    cols = torch.as_tensor(answers, dtype=torch.int64)
    soft = torch.softmax(logits, -1)
    inside = (cols >= 0) & (cols < A)
    at = soft.gather(-1, cols.clamp(0, A - 1).view(B, 1, 1, 1).expand(B, 2, K, 1))[..., 0]
    best = logits.max(-1).values
    top = (logits == best[..., None]).to(torch.int8).argmax(-1)       # the first column that holds the maximum
    if A > 1:
        margin = best - logits.scatter(-1, top[..., None], float("-inf")).max(-1).values
    else:
        margin = torch.full_like(best, float("inf"))
    return dict(prob=at * inside.view(B, 1, 1), top=top, top_prob=soft.gather(-1, top[..., None])[..., 0], margin=margin)


def brute_prob_curves(sd, do_option, vn, qf, img, answers, grid, order):
    """curve_stats of brute_logit_curves, with the logits under "logits"."""
    logits = brute_logit_curves(sd, do_option, vn, qf, img, grid, order)
    return dict(curve_stats(logits, answers), logits=logits)


def kernel_form_hidden(base, U, slot, probs, score, cnull, order):
    """What vqa_occl_curves_hidden computes, in float64: H [B, 2, P+1, hid].  The operands are faithfulness_ref
    .kernel_form_curves' without W2, b2 and answers."""
    base, U, probs, score, cnull = (x.double() for x in (base, U, probs, score, cnull))
    slot = torch.as_tensor(slot, dtype=torch.int64)
    B, G, P = probs.shape
    m = score.max(-1, keepdim=True).values
    r = (torch.exp(cnull.reshape(m.shape) - m) / torch.exp(score - m).sum(-1, keepdim=True))[..., 0]
    steps = torch.arange(P + 1, dtype=torch.float64)
    sides = []
    for mask, absent in zip(FR.kept_sets(order, P), (steps, P - steps)):
        mass = torch.einsum("bks,bgs->bgk", mask, probs)
        alpha = 1.0 / (mass + absent[None, None, :] * r[..., None])
        acc = torch.einsum("bks,bgs,bsgh->bgkh", mask, probs, U[slot])
        sides.append(torch.relu(base[:, None, :] + (alpha[..., None] * acc).sum(1)))
    return torch.stack(sides, 1)


def closed_operands(sd, do_option, vn, qf, img):
    """(base, U, slot, probs, score, cnull, W2, b2) in float64 from a state dict: v', q', cnull, U and base by their products,
    as faithfulness_ref.closed_curves forms them."""
    sd = R._sd64(sd)
    img = torch.as_tensor(img, dtype=torch.int64)
    vn, vp, qp, wx, bx, _dwv, _, mode = R.model_inputs(sd, do_option, vn, qf, img, torch.zeros(len(img), dtype=torch.int64))
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
    return base, U, img, probs, score, cnull, sd["classifier.lin2.weight"], sd["classifier.lin2.bias"]


def closed_logit_curves(sd, do_option, vn, qf, img, order):
    """logits [B, 2, P+1, A] by the kept form: kernel_form_hidden times W2 plus b2."""
    *operands, W2, b2 = closed_operands(sd, do_option, vn, qf, img)
    return kernel_form_hidden(*operands, order) @ W2.t() + b2


def comparable(margin, logit_bound):
    """(mask, share left out): an fp32 arg-max is compared with the float64 one only where the float64 margin between the
    best and the second logit exceeds four times the logit bound in force."""
    mask = margin > 4 * logit_bound
    return mask, 1.0 - float(mask.double().mean())


@functools.lru_cache(maxsize=None)
def _fixture_brute(do_option, order):
    f = R.fixture_case(do_option)
    return brute_logit_curves(f["golden"].sd, do_option, f["vn"], f["qf"], f["img"], f["grid"], torch.tensor(order))


def fixture_brute_logit_curves(do_option, order):
    """brute_logit_curves of the fixture's pairs (attribution_ref.fixture_case) for a ranking, computed once per (fixture,
    ranking) and shared by the tests that need it."""
    return _fixture_brute(do_option, tuple(tuple(int(s) for s in row) for row in torch.as_tensor(order).tolist()))
