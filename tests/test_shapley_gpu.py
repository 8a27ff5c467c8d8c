"""GPU: sampled Shapley maps -- vqa_occl_curves_orders against vqa_occl_curves bit for bit, vqa_shapley_accumulate against
float64 (tests/shapley_ref.py) and against the exact Shapley value where the orders enumerate it, and VqaNet.explain_shapley /
explain_shapley_pairs on the golden fixtures against the exact value from the state dict, with the bit-for-bit relations to
answer, explain_faithfulness, a widened float16 cache, a permuted, a split and a chunked batch."""
import functools

import pytest
import torch

from dl_vqa_amd import Shapley, shapley_orders, unique_questions
from tests import attribution_ref as R
from tests import shapley_ref as SR
from tests.curves_util import MODELS, _bound as _curve_bound, _fixture_run
from tests.explain_util import build, columns as _columns, within
from tests.golden_util import Golden, tiny_cfg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_within = functools.partial(within, label="parity-shapley")
A = SR.ANSWERS
CURVE_TOL = 3e-6        # what tests/test_faithfulness_gpu.py holds vqa_occl_curves to, relative to max|curve|


def _ops():
    from dl_vqa_amd import ops
    return ops


def _same(xs, ys):
    """Bit-equal tensors, a NaN (the standard error of one order) equal to a NaN."""
    return all(x.shape == y.shape and bool(((x == y) | (torch.isnan(x) & torch.isnan(y))).all()) and
               torch.equal(torch.signbit(x), torch.signbit(y)) for x, y in zip(xs, ys))


@functools.lru_cache(maxsize=None)
def _L():
    return _ops().occl_curves_chunk()


# (B, R, gh, gw, G, hid, M): one position and one order; P = 4 and P = 5 with the half of all orders (the exact value); several
# quads per lane with a tail; one step and one chunk more than a chunk / a workgroup of chunks; 26 x 26
def _shapes():
    L = _L()
    return [(3, 2, 1, 1, 1, 20, 1), (4, 3, 2, 2, 2, 20, 12), (3, 2, 1, 5, 1, 24, 60), (3, 2, 3, 4, 3, 1028, 3),
            (3, 2, 1, L + 1, 4, 1028, 2), (3, 2, 1, 4 * L + 1, 2, 520, 5), (2, 2, 26, 26, 2, 1024, 2)]


EXACT = (1, 2)          # the shapes whose orders are SR.half_orders: their mean IS the Shapley value
LARGE = 6


@functools.lru_cache(maxsize=None)
def _case(index):
    shape = _shapes()[index]
    c = SR.case(shape)
    if index in EXACT:
        c["orders"] = SR.half_orders(shape[2] * shape[3])
        assert c["orders"].shape[0] == shape[6]
    return shape, c


def _dev(c, perm=None, answers=None):
    hid = c["base"].shape[1]
    d = lambda t: (t if perm is None else t[perm]).to(DEV)
    cols = c["answers"] if answers is None else answers
    return dict(base=d(c["base"]), U=c["U"].to(DEV), slot=d(c["slot"]).to(torch.int32), probs=d(c["probs"]), score=d(c["score"]),
                cnull=d(c["cnull"]), W2=c["W2"].to(DEV)[:, :hid], b2=c["b2"].to(DEV), answers=d(cols).to(torch.int32))


def _curves(c, perm=None, answers=None, orders=None, **kw):
    orders = c["orders"] if orders is None else orders
    return _ops().occl_curves_orders(**_dev(c, perm, answers), orders=orders.to(DEV).to(torch.int32), **kw)


def _rank(orders):
    P = orders.shape[1]
    return torch.empty_like(orders).scatter_(1, orders, torch.arange(P).expand_as(orders)).to(DEV).to(torch.int32)


def _accumulate(c, curves, group=None, answers=None):
    """maps, stderr, empty from the curves [B, M, P+1] of the case's orders, folded `group` orders per launch."""
    ops, orders = _ops(), c["orders"]
    M, P = orders.shape
    B = curves[0].shape[0]
    group = M if group is None else group
    slot = c["slot"].to(DEV).to(torch.int32)
    cols = (c["answers"] if answers is None else answers).to(DEV).to(torch.int32)
    state = (torch.full((B, P), 5.0, device=DEV), torch.full((B, P), 5.0, device=DEV))       # m0 == 0 reads no state
    out, empty = None, torch.full((B,), 7.0, device=DEV)
    for m0 in range(0, M, group):
        n = min(group, M - m0)
        part = tuple(t[:, m0:m0 + n].contiguous() for t in curves)
        out = ops.shapley_accumulate(*part, _rank(orders[m0:m0 + n]), slot, cols, state, A, c["U"].shape[0], m0=m0,
                                     total=M if m0 + n == M else 0, empty=empty)
    torch.cuda.synchronize()
    return out[0], out[1], empty


# ----------------------------------------------------------------------------- the curves over (question, order) pairs
@pytest.mark.parametrize("index", range(7))
def test_occl_curves_orders_equals_occl_curves_per_order_bit_for_bit(index):
    shape, c = _case(index)
    B, P, M = shape[0], shape[2] * shape[3], shape[6]
    ops, orders = _ops(), c["orders"]
    deletion, insertion = _curves(c)
    torch.cuda.synchronize()
    assert deletion.shape == insertion.shape == (B, M, P + 1)
    dev = _dev(c)
    for m in range(M):
        one = ops.occl_curves(**dev, order=orders[m].expand(B, P).contiguous().to(DEV).to(torch.int32))
        assert torch.equal(deletion[:, m], one[0]) and torch.equal(insertion[:, m], one[1]), m
    # the empty image from both sides, the same bits for every order
    assert torch.equal(deletion[:, :, P], insertion[:, :, 0])
    assert torch.equal(insertion[:, :, 0], insertion[:, :1, 0].expand(B, M))
    # permuting the questions permutes the rows, bit for bit
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(5))
    shuffled = _curves(c, perm=perm)
    assert torch.equal(shuffled[0], deletion[perm.to(DEV)]) and torch.equal(shuffled[1], insertion[perm.to(DEV)])
    # a column out of range gives two rows of +0.0 per order and leaves the others as they were
    bad = c["answers"].clone()
    bad[0], bad[B - 1] = A, -1
    zero = _curves(c, answers=bad, out=(torch.full_like(deletion, 7.0), torch.full_like(insertion, 7.0)))
    for z, full in zip(zero, (deletion, insertion)):
        assert float(z[0].abs().max()) == 0.0 and float(z[B - 1].abs().max()) == 0.0
        assert not bool(torch.signbit(z[0]).any()) and torch.equal(z[1:B - 1], full[1:B - 1])


def test_occl_curves_orders_covers_a_slot_window_with_two_calls():
    shape = (6, 2, 5, 7, 2, 520, 3)
    c = SR.case(shape)
    c["slot"] = torch.tensor([0, 1, 1, 0, 1, 0])
    whole = _curves(c)
    out = (torch.full_like(whole[0], 7.0), torch.full_like(whole[1], 7.0))
    for r0 in (0, 1):
        one = dict(c, U=c["U"][r0:r0 + 1])
        _curves(one, slot0=r0, out=out)
        if r0 == 0:                                                   # the other image's questions were left alone
            assert all(bool((t[c["slot"].to(DEV) == 1] == 7.0).all()) for t in out)
            assert all(bool((t[c["slot"].to(DEV) == 0] != 7.0).all()) for t in out)
    assert torch.equal(out[0], whole[0]) and torch.equal(out[1], whole[1])
    # the accumulation leaves the questions outside the window alone too
    maps, err, empty = _accumulate(c, whole)
    state = (torch.zeros_like(maps), torch.zeros_like(maps))
    got = (torch.full_like(maps, 7.0), torch.full_like(maps, 7.0))
    base = torch.full_like(empty, 7.0)
    slot, cols = c["slot"].to(DEV).to(torch.int32), c["answers"].to(DEV).to(torch.int32)
    for r0 in (0, 1):
        _ops().shapley_accumulate(*whole, _rank(c["orders"]), slot, cols, state, A, 1, slot0=r0, total=3, out=got, empty=base)
        if r0 == 0:
            assert bool((got[0][slot == 1] == 7.0).all()) and bool((got[1][slot == 1] == 7.0).all())
            assert bool((base[slot == 1] == 7.0).all())
    assert torch.equal(got[0], maps) and torch.equal(got[1], err) and torch.equal(base, empty)


def test_occl_curves_orders_refuses_a_width_that_is_no_multiple_of_4():
    from dl_vqa_amd._lib import VqaHipError
    with pytest.raises(VqaHipError, match="vqa_occl_curves_orders.*multiple of 4"):
        _curves(SR.case((3, 2, 2, 2, 1, 18, 2)))


# ----------------------------------------------------------------------------- the accumulation against float64
@functools.lru_cache(maxsize=None)
def _reference(index):
    _, c = _case(index)
    e, deletion, insertion = SR.pair_estimates(*SR.operands(c), c["orders"])
    return SR.sampled(e) + (max(float(deletion.abs().max()), float(insertion.abs().max())), insertion[:, 0, 0])


@pytest.mark.parametrize("index", range(7))
def test_shapley_accumulate_matches_float64(index):
    """Every shape, 26 x 26 included, under the one bound: maps within 6e-6 max|curve| of the float64 mean: each estimate differences curve values that carry the curve kernels'
    3e-6 max|curve| bound each -- (d ins[k+1] - d ins[k] + d del[k] - d del[k+1]) / 2 <= 2 * 3e-6 -- and the mean of M such
    estimates keeps it.  stderr: an estimate off by at most that bound moves the root of the mean square by at most the bound
    / sqrt(M) ... / sqrt(M - 1), taken as the bound / sqrt(M) plus 1e-3 relative for the fp32 root, sums and division."""
    shape, c = _case(index)
    B, P, M = shape[0], shape[2] * shape[3], shape[6]
    want_maps, want_err, top, want_empty = _reference(index)
    curves = _curves(c)
    maps, err, empty = _accumulate(c, curves)
    tol = 2 * CURVE_TOL * top
    _within(f"{shape} maps vs float64", maps, want_maps, tol)
    _within(f"{shape} baseline vs float64", empty, want_empty, CURVE_TOL * top)
    assert torch.equal(empty, curves[1][:, 0, 0])
    if M == 1:
        assert bool(torch.isnan(err).all()) and bool(torch.isnan(want_err).all())
    else:
        diff = (err.double().cpu() - want_err).abs()
        allowed = tol / M ** 0.5 + 1e-3 * want_err
        print(f"[parity-shapley] {shape} stderr vs float64: max|diff| = {float(diff.max()):.3e}, max (diff / allowed) = "
              f"{float((diff / allowed).max()):.3f}, max stderr {float(want_err.max()):.3e}")
        assert bool((diff <= allowed).all())
    # the sums telescope: completeness up to rounding, whatever the orders
    full = curves[1][:, :, P].double().mean(1)
    gap = float((maps.double().sum(1) - (full - empty.double())).abs().max())
    print(f"[parity-shapley] {shape} completeness of the kernel's maps: {gap:.3e} (bound {P * tol:.3e})")
    assert gap <= P * tol
    # groups of 1, of 2 and of all orders: the same bits
    for group in (1, 2):
        assert _same(_accumulate(c, curves, group=group), (maps, err, empty))
    # a column out of range: +0.0 rows of maps, stderr and baseline; the other rows as they were
    bad = c["answers"].clone()
    bad[0], bad[B - 1] = A, -1
    zero = _accumulate(c, _curves(c, answers=bad), answers=bad)
    for z, full in zip(zero, (maps, err, empty)):
        z, full = z.view(B, -1), full.view(B, -1)
        assert float(z[0].abs().max()) == 0.0 and float(z[B - 1].abs().max()) == 0.0 and not bool(torch.signbit(z[0]).any())
        assert _same([z[1:B - 1]], [full[1:B - 1]])
    if index in EXACT:                                                # the half of all orders: the Shapley value itself
        _within(f"{shape} maps vs the exact Shapley value", maps, SR.exact(*SR.operands(c)), tol)


def test_shapley_accumulate_on_a_26_x_26_grid_from_its_own_curves():
    """Beside the float64 comparison above, a tighter one that isolates the accumulation from the 676 sequential adds of the
    curves: against float64 on the device's OWN curves an estimate takes three fp32 roundings of values below 2 max|curve|, the
    running mean one more per order: (3 + M) * 2^-24 * 2 max|curve|."""
    shape, c = _case(LARGE)
    M = shape[6]
    curves = _curves(c)
    maps, err, empty = _accumulate(c, curves)
    want_maps, want_err = SR.sampled(SR.estimates(curves[0].cpu(), curves[1].cpu(), c["orders"]))
    top = max(float(curves[0].abs().max()), float(curves[1].abs().max()))
    tol = (3 + M) * 2.0 ** -24 * 2 * top
    _within(f"{shape} maps vs float64 on the device's curves", maps, want_maps, tol)
    diff = (err.double().cpu() - want_err).abs()
    assert bool((diff <= tol / M ** 0.5 + 1e-3 * want_err).all())
    again = _accumulate(c, curves, group=1)
    assert torch.equal(again[0], maps) and torch.equal(again[1], err) and torch.equal(again[2], empty)


def test_sampled_maps_stay_within_four_standard_errors_of_the_exact_value():
    """A condition, not a measurement: 32 drawn orders at P = 6 against all 720 permutations; tests/test_shapley_cpu.py holds
    the float64 estimate of the same orders to 3 standard errors."""
    c = SR.case(SR.SAMPLING_SHAPE)
    P, M = 6, SR.SAMPLING_SHAPE[6]
    c["orders"] = shapley_orders(2 * M, P, SR.SAMPLING_SEED)
    exact = SR.exact(*SR.operands(c))
    _, ref_err = SR.sampled(SR.pair_estimates(*SR.operands(c), c["orders"])[0])
    maps, err, _ = _accumulate(c, _curves(c))
    ratio = (maps.double().cpu() - exact).abs() / ref_err
    print(f"[parity-shapley] P = 6, 32 orders of seed {SR.SAMPLING_SEED}: max |maps - exact| / stderr_ref = "
          f"{float(ratio.max()):.2f}")
    assert bool((ratio <= 4.0).all())


# ----------------------------------------------------------------------------- the whole path on the golden fixtures
@pytest.mark.parametrize("do_option,compute_dtype", MODELS)
def test_explain_shapley_matches_the_exact_value_and_its_siblings(do_option, compute_dtype):
    """maps within twice the absolute bound that tests/test_faithfulness_gpu.py holds explain_faithfulness's curves to on these
    fixtures (max(4 x answer()'s own error against float64, 1e-7): an estimate is half the sum of two differences of curve
    values); the completeness gap within P times that curve bound."""
    run = _fixture_run(do_option, compute_dtype)
    bound = _curve_bound(compute_dtype)
    m, feats, q, ql, img = run["m"], run["feats"], run["q"], run["ql"], run["img"]
    name = f"{R.FIXTURES[do_option]} {compute_dtype}"
    B, n_answers = run["full"].shape
    P = feats.vn.shape[1]
    assert P == 4
    table = SR.half_orders(P)
    for what, given in (("arg-max", None), ("given columns", _columns(B, n_answers))):
        res = m.explain_shapley(feats, q, ql, img, answers=given, orders=table)
        torch.cuda.synchronize()
        assert isinstance(res, Shapley) and res.maps.shape == res.stderr.shape == (B, *feats.grid)
        assert res.maps.dtype == res.stderr.dtype == res.baseline_logits.dtype == torch.float32
        assert res.answers.dtype == torch.int64 and res.answers.shape == res.baseline_logits.shape == (B,)
        assert not res.maps.requires_grad and m._last_ctx is None
        assert torch.equal(res.logits, run["full"])                   # answer()'s, bit for bit
        cols = res.answers.tolist()
        assert cols == (run["full"].argmax(1).tolist() if given is None else given)
        _within(f"{name} {what} maps vs the exact Shapley value (bound 2 x {bound:.3e})", res.maps.reshape(B, P),
                SR.fixture_exact(do_option, cols), 2 * bound)
        gap = res.completeness_gap()
        assert gap.dtype == torch.float64 and gap.shape == (B,)
        _within(f"{name} {what} completeness gap (bound P x {bound:.3e})", gap, torch.zeros(B, dtype=torch.float64), P * bound)
        assert bool((res.stderr >= 0).all())
        faith = m.explain_faithfulness(feats, q, ql, img, torch.zeros(B, P), answers=given)
        assert torch.equal(res.baseline_logits, faith.insertion[:, 0])


@pytest.mark.parametrize("do_option,compute_dtype", MODELS)
def test_explain_shapley_relations(do_option, compute_dtype):
    run = _fixture_run(do_option, compute_dtype)
    m, feats, q, ql, img = run["m"], run["feats"], run["q"], run["ql"], run["img"]
    B, n_answers = run["full"].shape
    P = feats.vn.shape[1]
    same = _same
    res = m.explain_shapley(feats, q, ql, img, permutations=8, seed=3)
    # the drawn table is shapley_orders'
    assert same(res, m.explain_shapley(feats, q, ql, img, orders=shapley_orders(8, P, 3)))
    assert same(res, m.explain_shapley(feats, q, ql, img, orders=shapley_orders(8, P, 3).to(torch.int32).to(DEV)))
    assert not torch.equal(res.maps, m.explain_shapley(feats, q, ql, img, permutations=8, seed=4).maps)
    assert bool(torch.isnan(m.explain_shapley(feats, q, ql, img, permutations=2).stderr).all())
    # a CUDA column out of range: +0.0 rows, the other rows untouched
    bad = res.answers.clone()
    bad[2] = n_answers
    zero = m.explain_shapley(feats, q, ql, img, answers=bad, permutations=8, seed=3)
    for z, full in ((zero.maps, res.maps), (zero.stderr, res.stderr), (zero.baseline_logits, res.baseline_logits)):
        assert float(z[2].abs().max()) == 0.0 and not bool(torch.signbit(z[2]).any())
        assert torch.equal(z[:2], full[:2]) and torch.equal(z[3:], full[3:])
    # one image per chunk of U, one order per launch: the same bits
    per_image = P * m._engine.G * m._engine.hid * 4
    assert same(res, m.explain_shapley(feats, q, ql, img, permutations=8, seed=3, _u_bytes=per_image, _ws_bytes=1))
    assert same(res, m.explain_shapley(feats, q, ql, img, permutations=8, seed=3, _ws_bytes=1))
    two = 2 * _ops()._lib.load().vqa_occl_curves_orders_workspace_bytes(B, 1, P, m._engine.G, m._engine.hid)
    assert same(res, m.explain_shapley(feats, q, ql, img, permutations=8, seed=3, _ws_bytes=two + 4))
    # a permuted batch and a split batch: the same rows, bit for bit
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(3))
    pd = perm.to(DEV)
    shuffled = m.explain_shapley(feats, q[pd], ql[pd], [img[i] for i in perm.tolist()], permutations=8, seed=3)
    assert same(shuffled, [t[pd] for t in res])
    for b0, b1 in ((0, 3), (3, B)):
        part = m.explain_shapley(feats, q[b0:b1], ql[b0:b1], img[b0:b1], permutations=8, seed=3)
        assert same(part, [t[b0:b1] for t in res])
    # the same pairs from the two caches
    qu, qlu, qidx = unique_questions(run["f"]["q"], run["f"]["q_len"])
    qfeats = m.encode_questions(qu.to(DEV), qlu.to(DEV))
    pairs = m.explain_shapley_pairs(feats, qfeats, img, qidx, permutations=8, seed=3)
    assert torch.equal(pairs.logits, m.answer_pairs(feats, qfeats, img, qidx))
    name = f"{R.FIXTURES[do_option]} {compute_dtype}"
    bitwise = torch.equal(pairs.logits, res.logits)
    print(f"[parity-shapley] {name}: answer_pairs logits are answer's bit for bit: {bitwise}")
    if bitwise:
        assert same(pairs, res)
    else:                                                             # whatever relation answer_pairs has to answer, within bounds
        bound = _curve_bound(compute_dtype)
        assert float((pairs.logits - res.logits).abs().max()) <= bound
        given = m.explain_shapley_pairs(feats, qfeats, img, qidx, answers=res.answers, permutations=8, seed=3)
        assert torch.equal(given.answers, res.answers)
        _within(f"{name} explain_shapley_pairs vs explain_shapley, maps", given.maps, res.maps, 2 * bound)
        _within(f"{name} explain_shapley_pairs vs explain_shapley, baseline_logits", given.baseline_logits, res.baseline_logits,
                bound)
        # M = 4 orders: estimates off by at most 2 x bound move |e - mean| by at most sqrt(M) times that, hence the standard
        # error by at most 2 x bound / sqrt(M - 1)
        _within(f"{name} explain_shapley_pairs vs explain_shapley, stderr", given.stderr, res.stderr, 2 * bound / 3 ** 0.5)
    # a float16 cache gives its widened copy's results
    if compute_dtype == "fp32":
        f16 = feats.to(torch.float16)
        f32 = f16.to(torch.float32)
        assert same(m.explain_shapley(f16, q, ql, img, permutations=8, seed=3),
                    m.explain_shapley(f32, q, ql, img, permutations=8, seed=3))
        assert same(m.explain_shapley_pairs(f16, qfeats, img, qidx, permutations=8, seed=3),
                    m.explain_shapley_pairs(f32, qfeats, img, qidx, permutations=8, seed=3))
    # an empty batch
    for none in (m.explain_shapley(feats, q[:0], ql[:0], []), m.explain_shapley_pairs(feats, qfeats, [], [])):
        assert isinstance(none, Shapley) and none.maps.shape == none.stderr.shape == (0, *feats.grid)
        assert none.answers.shape == none.baseline_logits.shape == (0,) and none.answers.dtype == torch.int64
        assert none.logits.shape == (0, n_answers) and none.completeness_gap().shape == (0,)
    assert m._last_ctx is None and all(p.grad is None for p in m.parameters())


def test_forward_and_backward_are_unchanged_after_explain_shapley():
    from dl_vqa_amd.train import soft_ce_loss_and_score
    g = Golden("tiny_plus")
    cfg = tiny_cfg(g.meta)
    v, q, ql = g.t["v"].to(DEV), g.t["q"].to(DEV), g.t["q_len"].to(DEV)
    a_idx, a_val = g.t["a_idx"].to(DEV), g.t["a_val"].to(DEV)

    def step(m):
        y = m(v, q, ql)
        soft_ce_loss_and_score(y, a_idx, a_val)[0].backward()
        torch.cuda.synchronize()
        return y.detach().clone(), {k: p.grad.clone() for k, p in m.named_parameters()}

    fresh = build(cfg, g.meta["V"], g.sd).eval()
    y0, g0 = step(fresh)

    m = build(cfg, g.meta["V"], g.sd).eval()
    m._ensure_flat()
    flat_grad = m._flat_grad
    flat_grad.fill_(3.0)
    torch.manual_seed(77)
    rng = torch.get_rng_state()
    feats = m.encode_images(v)
    idx = list(range(q.shape[0]))
    got = m.explain_shapley(feats, q, ql, idx)
    torch.cuda.synchronize()
    assert torch.equal(got.logits, m.answer(feats, q, ql, idx)) and float(got.maps.abs().max()) > 1e-4
    assert m._last_ctx is None and len(m._pending) == 0
    assert m._flat_grad is flat_grad and bool((flat_grad == 3.0).all())
    assert torch.equal(torch.get_rng_state(), rng)                  # neither seed stream was drawn from
    assert all(p.grad is None for p in m.parameters())
    flat_grad.zero_()
    y1, g1 = step(m)
    assert torch.equal(y1, y0)
    for k in g0:
        assert torch.equal(g1[k], g0[k]), k
    # refusals that need a device: foreign features, an index outside the cache
    with pytest.raises(RuntimeError, match="belong elsewhere"):
        fresh.explain_shapley(feats, q, ql, idx)
    with pytest.raises(IndexError):
        m.explain_shapley(feats, q, ql, idx[:-1] + [feats.N])
