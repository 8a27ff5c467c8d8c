"""float64 references for the sampled Shapley maps of VqaNet.explain_shapley / explain_shapley_pairs (include/vqa_hip.h
vqa_occl_curves_orders, vqa_shapley_accumulate):

  all_orders / half_orders   every permutation of 0 .. P-1, and the half with pi[0] < pi[-1] (one of each reversal pair);
  curves_for_orders          faithfulness_ref.kernel_form_curves over (question, order) pairs: [B, M, P+1];
  estimates                  e_m[b, p] from curves: the mean of p's marginal under orders[m] and under its reverse;
  pair_estimates             the two together, from the operands the entry point takes;
  sampled                    mean and standard error over the orders (NaN for one order);
  exact                      the Shapley value itself, by the insertion marginals of ALL permutations (P <= 6);
  exact_from_state_dict      the same from a state dict, via faithfulness_ref.closed_curves or brute_curves.

Everything here runs on the CPU; the GPU tests import it and compute each reference once."""
import functools
import itertools

import torch

from tests import attribution_ref as R
from tests import faithfulness_ref as FR


ANSWERS = 11
SAMPLING_SHAPE = (3, 2, 2, 3, 2, 20, 32)      # P = 6: 32 drawn orders against all 720
SAMPLING_SEED = 0                             # test_shapley_cpu checks that the float64 reference stays within 3 stderr


def case(shape, seed_offset=0):
    """Consistent synthetic operands of vqa_occl_curves_orders for shape (B, R, gh, gw, G, hid, M), built the way
    tests/curves_util.py builds vqa_occl_curves': probs = softmax(score), cnull = the row's log-sum-exp + log r with r
    drawn from [1/15, 0.6], the questions spread over the R images; orders: M random permutations."""
    import math
    B, Rr, gh, gw, G, hid, M = shape
    P = gh * gw
    g = torch.Generator().manual_seed(1000 * B + 100 * gh + 10 * G + gw + hid + 7 * M + seed_offset)
    slot = torch.randint(0, Rr, (B,), generator=g)
    score = 2 * torch.randn(B, G, P, generator=g)
    orders = torch.stack([torch.randperm(P, generator=g) for _ in range(M)])
    lo, hi = 1.0 / 15.0, 0.6
    r = torch.exp(math.log(lo) + (math.log(hi) - math.log(lo)) * torch.rand(B, G, generator=g))
    probs = torch.softmax(score, dim=-1)
    U = torch.randn(Rr, P, G, hid, generator=g)
    base = torch.randn(B, hid, generator=g)
    cnull = (torch.logsumexp(score.double(), -1) + torch.log(r.double())).float()
    W2 = torch.randn(ANSWERS, hid + 4, generator=g)                   # a leading dimension wider than the rows
    b2 = torch.randn(ANSWERS, generator=g)
    answers = torch.randint(0, ANSWERS, (B,), generator=g)
    return dict(base=base, U=U, slot=slot, probs=probs, score=score, cnull=cnull, W2=W2, b2=b2, answers=answers, orders=orders)


def operands(c):
    """The case's operands in the order of the reference functions here (W2 without its padding columns)."""
    hid = c["base"].shape[1]
    return (c["base"], c["U"], c["slot"], c["probs"], c["score"], c["cnull"], c["W2"][:, :hid], c["b2"], c["answers"])


def all_orders(P):
    assert P <= 6, "P! orders: enumeration is for tiny grids"
    return torch.tensor(list(itertools.permutations(range(P))), dtype=torch.int64).reshape(-1, P)


def half_orders(P):
    """One order of every (order, reversed order) pair: those with pi[0] < pi[-1]; all of them for P == 1."""
    full = all_orders(P)
    return full if P == 1 else full[full[:, 0] < full[:, -1]]


def curves_for_orders(base, U, slot, probs, score, cnull, W2, b2, answers, orders):
    """(deletion, insertion) [B, M, P+1] in float64: row (b, m) is kernel_form_curves of question b along orders[m]."""
    orders = torch.as_tensor(orders, dtype=torch.int64)
    M, P = orders.shape
    B = probs.shape[0]
    rep = lambda t: torch.as_tensor(t).repeat_interleave(M, 0)
    out = FR.kernel_form_curves(rep(base), U, rep(slot), rep(probs), rep(score), rep(torch.as_tensor(cnull).reshape(B, -1)), W2, b2,
                                rep(answers), orders.repeat(B, 1))
    return out["deletion"].view(B, M, P + 1), out["insertion"].view(B, M, P + 1)


def estimates(deletion, insertion, orders):
    """e [B, M, P]: e[b, m, orders[m, k]] = ((ins[k+1] - ins[k]) + (del[k] - del[k+1])) / 2 from curves [B, M, P+1]."""
    orders = torch.as_tensor(orders, dtype=torch.int64)
    deletion, insertion = deletion.double(), insertion.double()
    steps = 0.5 * ((insertion[..., 1:] - insertion[..., :-1]) + (deletion[..., :-1] - deletion[..., 1:]))
    return torch.zeros_like(steps).scatter_(2, orders[None].expand_as(steps), steps)


def pair_estimates(base, U, slot, probs, score, cnull, W2, b2, answers, orders):
    """(e [B, M, P], deletion, insertion [B, M, P+1]) in float64 from the operands of vqa_occl_curves_orders."""
    deletion, insertion = curves_for_orders(base, U, slot, probs, score, cnull, W2, b2, answers, orders)
    return estimates(deletion, insertion, orders), deletion, insertion


def sampled(e):
    """(maps, stderr) [B, P] of the estimates e [B, M, P]: the mean over the orders and sqrt(sum (e - mean)^2 / (M (M - 1))),
    NaN for M == 1."""
    M = e.shape[1]
    mean = e.mean(1)
    if M == 1:
        return mean, torch.full_like(mean, float("nan"))
    return mean, (((e - mean[:, None]) ** 2).sum(1) / (M * (M - 1))).sqrt()


def exact(base, U, slot, probs, score, cnull, W2, b2, answers):
    """The Shapley value [B, P] of f_b(S) = the kept-form logit with the positions S present: the marginal contribution of each
    position along the insertion curve, averaged over ALL P! permutations."""
    orders = all_orders(probs.shape[2])
    _, insertion = curves_for_orders(base, U, slot, probs, score, cnull, W2, b2, answers, orders)
    steps = insertion[..., 1:] - insertion[..., :-1]
    return torch.zeros_like(steps).scatter_(2, orders[None].expand_as(steps), steps).mean(1)


def curves_from_state_dict(sd, do_option, vn, qf, img, answers, grid, orders, brute=False):
    """(deletion, insertion) [B, M, P+1] from a state dict: closed_curves (the kept form), or brute_curves (a forward per kept
    set) when brute."""
    B = len(img)
    out = ([], [])
    for row in torch.as_tensor(orders, dtype=torch.int64):
        order = row[None].expand(B, -1)
        curves = (FR.brute_curves if brute else FR.closed_curves)(sd, do_option, vn, qf, img, answers, grid, order)
        out[0].append(curves[0]), out[1].append(curves[1])
    return torch.stack(out[0], 1), torch.stack(out[1], 1)


def exact_from_state_dict(sd, do_option, vn, qf, img, answers, grid, brute=False):
    """The Shapley value [B, P] from a state dict, by the insertion marginals of all P! permutations."""
    orders = all_orders(vn.shape[1])
    _, insertion = curves_from_state_dict(sd, do_option, vn, qf, img, answers, grid, orders, brute)
    steps = insertion[..., 1:] - insertion[..., :-1]
    return torch.zeros_like(steps).scatter_(2, orders[None].expand_as(steps), steps).mean(1)


@functools.lru_cache(maxsize=None)
def _fixture_exact(do_option, answers):
    f = R.fixture_case(do_option)
    return exact_from_state_dict(f["golden"].sd, do_option, f["vn"], f["qf"], f["img"], list(answers), f["grid"])


def fixture_exact(do_option, answers):
    """exact_from_state_dict of the fixture's pairs (attribution_ref.fixture_case) for the given answer columns, computed once
    per (fixture, columns) and shared by the tests that need it."""
    return _fixture_exact(do_option, tuple(int(a) for a in answers))
