"""What the tests of the calls that explain sets of grid positions share (test_occlusion_*, test_faithfulness_*,
test_prob_curves_*, test_shapley_*): the random float64 case and maps of the CPU tests; the synthetic operands of the curve
kernels, the fixture runs, the brute-force route on the device and the whole-path bound of the GPU tests.  A plain module: no
fixture, no pytest setting; nothing here touches a device until it is called."""
import functools
import math

import torch

from dl_vqa_amd import ImageFeatures
from tests import attribution_ref as R
from tests import faithfulness_ref as FR
from tests.explain_util import columns as _columns, fixture_model as _fixture_model, grouping as _grouping

DEV = "cuda:0"
A = 11


# ----------------------------------------------------------------------------- CPU: float64 cases
def _random_case(do_option, G, grid, seed):
    """A random attention stage + classifier in float64 (state-dict names and shapes of the model) and random inputs, with
    weights of a size that keeps the logits O(1)."""
    g = torch.Generator().manual_seed(seed)
    N, B, C, mid, Q, hid, A = 3, 5, 10, 12, 6, 9, 5
    gh, gw = grid
    xld = 2 * mid if do_option == "|" else mid
    rn = lambda *s: 0.5 * torch.randn(*s, generator=g, dtype=torch.float64)
    sd = {"attention.v_conv.weight": rn(mid, C, 1, 1), "attention.q_lin.weight": rn(mid, Q), "attention.q_lin.bias": rn(mid),
          "attention.x_conv.weight": rn(G, xld, 1, 1), "attention.x_conv.bias": rn(G),
          "classifier.lin1.weight": rn(hid, G * C + Q), "classifier.lin1.bias": rn(hid),
          "classifier.lin2.weight": rn(A, hid), "classifier.lin2.bias": rn(A)}
    vn = torch.randn(N, gh * gw, C, generator=g, dtype=torch.float64)
    vn = vn / vn.norm(dim=-1, keepdim=True)
    qf = torch.randn(B, Q, generator=g, dtype=torch.float64)
    img = torch.randint(0, N, (B,), generator=g)
    answers = torch.randint(0, A, (B,), generator=g)
    return sd, vn, qf, img, answers


def _maps(B, P, seed, ties):
    g = torch.Generator().manual_seed(seed)
    if ties:                                                          # three distinct values and a signed zero
        m = torch.randint(-1, 2, (B, P), generator=g).double()
        m[:, 0] = -0.0
        return m
    return torch.randn(B, P, generator=g, dtype=torch.float64)


# ----------------------------------------------------------------------------- GPU: the curve kernels on synthetic operands
def _ops():
    from dl_vqa_amd import ops
    return ops


@functools.lru_cache(maxsize=None)
def _L():
    return _ops().occl_curves_chunk()


def _case(shape, kind, concentrate=None):
    """Consistent synthetic operands of vqa_occl_curves: probs = softmax(score), cnull = the row's log-sum-exp + log r with r
    drawn from [1/15, 0.6], a random ranking per question.  concentrate = r: questions 0 and 1 hold 0.99 of every glimpse's mass
    on one position, ranked last by question 0 and first by question 1, and every question has that r."""
    B, Rr, gh, gw, G, hid = shape
    P = gh * gw
    g = torch.Generator().manual_seed(1000 * B + 100 * gh + 10 * G + gw + hid)
    slot = _grouping(kind, Rr, B, g) if Rr > 1 else torch.zeros(B, dtype=torch.int64)
    score = 2 * torch.randn(B, G, P, generator=g)
    order = torch.stack([torch.randperm(P, generator=g) for _ in range(B)])
    lo, hi = 1.0 / 15.0, 0.6
    r = torch.exp(math.log(lo) + (math.log(hi) - math.log(lo)) * torch.rand(B, G, generator=g))
    if concentrate is not None:
        star = P // 2
        for b in (0, 1):
            others = torch.cat([score[b, :, :star], score[b, :, star + 1:]], -1).double()
            score[b, :, star] = (torch.logsumexp(others, -1) + math.log(99.0)).float()
            rest = order[b][order[b] != star]
            order[b] = torch.cat([rest, torch.tensor([star])]) if b == 0 else torch.cat([torch.tensor([star]), rest])
        r[:] = concentrate
    probs = torch.softmax(score, dim=-1)
    U = torch.randn(Rr, P, G, hid, generator=g)
    base = torch.randn(B, hid, generator=g)
    cnull = (torch.logsumexp(score.double(), -1) + torch.log(r.double())).float()
    W2 = torch.randn(A, hid + 4, generator=g)                         # a leading dimension wider than the rows
    b2 = torch.randn(A, generator=g)
    answers = torch.randint(0, A, (B,), generator=g)
    return dict(base=base, U=U, slot=slot, probs=probs, score=score, cnull=cnull, W2=W2, b2=b2, answers=answers, order=order)


def _run(c, perm=None, answers=None, order=None, out=None, U=None, slot0=0):
    ops = _ops()
    hid = c["base"].shape[1]
    d = lambda t: (t if perm is None else t[perm]).to(DEV)
    cols = c["answers"] if answers is None else answers
    rank = c["order"] if order is None else order
    return ops.occl_curves(d(c["base"]), (c["U"] if U is None else U).to(DEV), d(c["slot"]).to(torch.int32), d(c["probs"]),
                           d(c["score"]), d(c["cnull"]), c["W2"].to(DEV)[:, :hid], c["b2"].to(DEV), d(cols).to(torch.int32),
                           d(rank).to(torch.int32), slot0=slot0, out=out)


# ----------------------------------------------------------------------------- GPU: the whole path on the golden fixtures
MODELS = [("+", "fp32"), ("*", "fp32"), ("|", "fp32"), ("+", "fp32x3"), ("*", "fp32x3"), ("|", "fp32x3")]


@functools.lru_cache(maxsize=None)
def _fixture_run(do_option, compute_dtype):
    f, m, feats = _fixture_model(do_option, compute_dtype)
    q, ql, img = f["q"].to(DEV), f["q_len"].to(DEV), list(R.IMAGE_INDEX)
    full = m.answer(feats, q, ql, img)
    torch.cuda.synchronize()
    return dict(f=f, m=m, feats=feats, q=q, ql=ql, img=img, full=full)


def _picked(t, cols):
    """t[..., A] at each question's column."""
    idx = torch.as_tensor(cols, dtype=torch.int64, device=t.device)
    return t.gather(-1, idx.view(-1, *([1] * (t.dim() - 1))).expand(*t.shape[:-1], 1))[..., 0]


def _device_brute(run, order):
    """The brute-force route on the device: answer() on a bank that holds one copy of its image per question, with the rows of
    every kept set's complement zeroed in vn and in v'.  Returns (deletion, insertion) logits [B, P+1, A]."""
    m, feats, q, ql, img = run["m"], run["feats"], run["q"], run["ql"], run["img"]
    N, P, C = feats.vn.shape
    B = len(img)
    pick = torch.tensor(img, device=DEV)
    vn, vp = feats.vn[pick], feats.vprime.view(N, P, -1)[pick]
    out = []
    for mask in FR.kept_sets(order, P):
        keep = mask.to(DEV).float()                                   # [B, P+1, P]
        curve = [m.answer(ImageFeatures((vn * keep[:, k, :, None]).contiguous(),
                                        (vp * keep[:, k, :, None]).reshape(B * P, -1).contiguous(), feats.grid, m),
                          q, ql, list(range(B))) for k in range(P + 1)]
        out.append(torch.stack(curve, 1))
    torch.cuda.synchronize()
    return tuple(out)


def _tied_map(B, P):
    g = torch.Generator().manual_seed(B + P)
    return torch.randint(0, 2, (B, P), generator=g).float()          # two values: ties everywhere


@functools.lru_cache(maxsize=None)
def _bound(compute_dtype):
    """The tolerance of the whole-path tests, measured on code that is not under test: the largest absolute difference, over
    the three fixtures, the arg-max and the given columns, between answer() on the zeroed banks (the ranking of a fixed map
    with ties) and the float64 brute force, times 4 -- the kept form forms the same sums in another order, with one division
    more -- and not below 1e-7 (one ulp of a 0.27 logit is 3e-8)."""
    worst = 0.0
    for do_option in ("+", "*", "|"):
        run = _fixture_run(do_option, compute_dtype)
        B, n_answers = run["full"].shape
        order = FR.rank_desc(_tied_map(B, run["feats"].vn.shape[1]))
        device = _device_brute(run, order)
        for cols in (run["full"].argmax(1).tolist(), _columns(B, n_answers)):
            for got, want in zip(device, FR.fixture_brute_curves(do_option, cols, order)):
                worst = max(worst, float((_picked(got, cols).double().cpu() - want).abs().max()))
    bound = max(4 * worst, 1e-7)
    print(f"[parity-faithfulness] {compute_dtype}: answer() on zeroed banks vs float64 brute force, max|diff| over the three "
          f"fixtures = {worst:.3e}; whole-path bound = max(4 x that, 1e-7) = {bound:.3e}")
    return bound
