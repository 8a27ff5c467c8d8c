"""GPU: deletion and insertion curves of an attribution map -- vqa_rank_desc against the reference ranking, vqa_occl_curves
against float64 (tests/faithfulness_ref.py) on synthetic inputs, and VqaNet.explain_faithfulness / explain_faithfulness_pairs on
the golden fixtures against the brute-force route on the device (answer() on per-question banks with the absent rows zeroed) and
against the float64 brute force, with the bit-for-bit relations to answer, a widened float16 cache and a permuted batch."""
import functools

import pytest
import torch

from dl_vqa_amd import Faithfulness, unique_questions
from tests import attribution_ref as R
from tests import faithfulness_ref as FR
from tests.curves_util import MODELS, A, _bound, _case, _device_brute, _fixture_run, _L, _ops, _picked, _run, _tied_map
from tests.explain_util import build, columns as _columns, rel, within
from tests.golden_util import Golden, tiny_cfg
from tests.test_kernels_gpu import check

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_within = functools.partial(within, label="parity-faithfulness")


# ----------------------------------------------------------------------------- the ranking
def _rank_rows(B, P, seed):
    """Rows with ties, signed zeros, NaN and -inf among random values, and (row 0) a constant row."""
    g = torch.Generator().manual_seed(seed)
    maps = torch.randn(B, P, generator=g)
    kind = torch.randint(0, 8, (B, P), generator=g)
    maps = torch.where(kind == 0, torch.zeros(()), maps)
    maps = torch.where(kind == 1, -torch.zeros(()), maps)
    maps = torch.where(kind == 2, torch.full((), float("nan")), maps)
    maps = torch.where(kind == 3, torch.round(maps), maps)            # ties
    maps = torch.where((kind == 4) & (maps > 1.5), torch.full((), float("-inf")), maps)
    maps[0] = 0.25
    return maps


@pytest.mark.parametrize("B", [1, 7])
@pytest.mark.parametrize("P", [1, 4, 35, 676, 8192])
def test_rank_desc_matches_the_reference(P, B):
    maps = _rank_rows(B, P, 10 * P + B)
    order = _ops().rank_desc(maps.to(DEV))
    torch.cuda.synchronize()
    assert order.dtype == torch.int32 and order.shape == (B, P)
    assert torch.equal(order.cpu().long(), FR.rank_desc(maps))
    assert order[0].tolist() == list(range(P))
    plain = torch.randn(B, P, generator=torch.Generator().manual_seed(P))
    assert torch.equal(_ops().rank_desc(plain.to(DEV)).cpu().long(), FR.rank_desc(plain))


def test_rank_desc_refuses_more_than_8192_positions():
    from dl_vqa_amd._lib import VqaHipError
    with pytest.raises(VqaHipError, match="P=8193"):
        _ops().rank_desc(torch.zeros(1, 8193, device=DEV))


# ----------------------------------------------------------------------------- the curve kernel against float64
# (B, R, gh, gw, G, hid): one position; hid of one and of several quads per lane, with and without a tail; G = 1..4; grids of
# one chunk, of several chunks per workgroup and (5 x 13, 26 x 26) of several workgroups per question
def _shapes():
    L = _L()
    return [(3, 2, 1, 1, 1, 20), (4, 3, 2, 2, 2, 20), (3, 2, 3, 4, 3, 1028), (3, 2, 5, 7, 2, 1024), (3, 2, 5, 7, 4, 520),
            (3, 2, 5, 7, 1, 1028), (3, 2, 1, L - 1, 2, 520), (3, 2, 1, L, 3, 1024), (3, 2, 1, L + 1, 4, 1028),
            (3, 2, 1, 4 * L + 1, 2, 520)]


LARGE = (2, 2, 26, 26, 2, 1024)


def _reference(c, order=None):
    hid = c["base"].shape[1]
    return FR.kernel_form_curves(c["base"], c["U"], c["slot"], c["probs"], c["score"], c["cnull"], c["W2"][:, :hid], c["b2"],
                                 c["answers"], c["order"] if order is None else order)


def _errors(tag, got, ref, tol):
    """Both curves against float64, each relative to its own largest value; returns the larger error."""
    deletion, insertion = (t.double().cpu() for t in got)
    check(f"occl_curves {tag} deletion", deletion, ref["deletion"], tol)
    check(f"occl_curves {tag} insertion", insertion, ref["insertion"], tol)
    return max(rel(deletion, ref["deletion"]), rel(insertion, ref["insertion"]))


def _check_kernel(shape, kind, tol=3e-6):
    c = _case(shape, kind)
    B, P = shape[0], shape[2] * shape[3]
    ref = _reference(c)
    alphas = torch.cat([ref["alpha_del"].flatten(), ref["alpha_ins"].flatten()])
    print(f"[parity-faithfulness] {shape} {kind}: alpha in [{float(alphas.min()):.3f}, {float(alphas.max()):.3f}]")
    got = _run(c)
    torch.cuda.synchronize()
    _errors(f"{shape} {kind}", got, ref, tol)
    deletion, insertion = got
    # the empty image, from both sides; the full image by both routes
    assert torch.equal(deletion[:, P], insertion[:, 0])
    # permuting the questions permutes the rows, bit for bit
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(5))
    shuffled = _run(c, perm=perm)
    assert torch.equal(shuffled[0], deletion[perm.to(DEV)]) and torch.equal(shuffled[1], insertion[perm.to(DEV)])
    # a column out of range gives two rows of +0.0 and leaves the others as they were
    bad = c["answers"].clone()
    bad[0], bad[B - 1] = A, -1
    zero = _run(c, answers=bad, out=(torch.full_like(deletion, 7.0), torch.full_like(insertion, 7.0)))
    for z, full in zip(zero, got):
        assert float(z[0].abs().max()) == 0.0 and float(z[B - 1].abs().max()) == 0.0
        assert not bool(torch.signbit(z[0]).any()) and torch.equal(z[1:B - 1], full[1:B - 1])
    return c, got


@pytest.mark.parametrize("kind", ["empty", "single", "shuffled"])
@pytest.mark.parametrize("index", range(10))
def test_occl_curves_matches_float64(index, kind):
    shapes = _shapes()
    assert len(shapes) == 10
    _check_kernel(shapes[index], kind)


def test_occl_curves_covers_a_slot_window_smaller_than_the_images_with_two_calls():
    shape = (6, 2, 5, 7, 2, 520)
    c = _case(shape, "shuffled")
    assert set(c["slot"].tolist()) == {0, 1}
    whole = _run(c)
    out = (torch.full_like(whole[0], 7.0), torch.full_like(whole[1], 7.0))
    for r0 in (0, 1):
        _run(c, U=c["U"][r0:r0 + 1], slot0=r0, out=out)
        if r0 == 0:                                                   # the other image's questions were left alone
            assert all(bool((t[c["slot"].to(DEV) == 1] == 7.0).all()) for t in out)
            assert all(bool((t[c["slot"].to(DEV) == 0] != 7.0).all()) for t in out)
    assert torch.equal(out[0], whole[0]) and torch.equal(out[1], whole[1])


def test_an_order_entry_out_of_range_adds_nothing_and_is_no_address():
    shape = (3, 2, 5, 7, 2, 520)
    c = _case(shape, "shuffled")
    order = c["order"].clone()
    order[0, 3], order[0, 20], order[1, 0], order[2, 34] = -1, 35, 2 ** 31 - 1, -(2 ** 31)
    got = _run(c, order=order)
    torch.cuda.synchronize()
    _errors("entries out of range", got, _reference(c, order), 3e-6)


def test_occl_curves_matches_float64_on_a_26_x_26_grid():
    """676 sequential adds have no project bound: the bound is four times what an fp32 restatement of the same sequential sums
    on the host (torch, not the code under test) loses against float64, and not below the project's 3e-6."""
    c = _case(LARGE, "shuffled")
    hid = c["base"].shape[1]
    ref = _reference(c)
    host = FR.sequential_curves(c["base"], c["U"], c["slot"], c["probs"], c["score"], c["cnull"], c["W2"][:, :hid], c["b2"],
                                c["answers"], c["order"], _L(), torch.float32)
    host_err = max(rel(host[0], ref["deletion"]), rel(host[1], ref["insertion"]))
    tol = max(3e-6, 4 * host_err)
    got = _run(c)
    torch.cuda.synchronize()
    err = _errors(f"{LARGE}", got, ref, tol)
    print(f"[parity-faithfulness] 26 x 26: fp32 host restatement vs float64 {host_err:.3e}, bound max(3e-6, 4 x that) = {tol:.3e}, "
          f"kernel vs float64 {err:.3e}")
    assert torch.equal(got[0][:, 676], got[1][:, 0])
    perm = torch.tensor([1, 0])
    shuffled = _run(c, perm=perm)
    assert torch.equal(shuffled[0], got[0][perm.to(DEV)]) and torch.equal(shuffled[1], got[1][perm.to(DEV)])


@pytest.mark.parametrize("r", [1e-1, 1e-2, 1e-4])
def test_occl_curves_keeps_its_bound_when_a_kept_set_holds_a_hundredth_of_the_mass(r):
    """The kept form has no cancellation: with 0.99 of every glimpse's mass on one position that is ranked last (question 0:
    every insertion set before the last holds at most 0.01) or first (question 1: every deletion set after the first does),
    the project's relative bound holds at every r; no alpha condition is needed."""
    c = _case((3, 2, 5, 7, 2, 1024), "shuffled", concentrate=r)
    ref = _reference(c)
    assert abs(float(c["probs"][0, 0, 17]) - 0.99) < 1e-4 and c["order"][0, -1] == 17 and c["order"][1, 0] == 17
    assert float((ref["r"] - r).abs().max()) < 1e-5 * r
    alphas = torch.cat([ref["alpha_del"].flatten(), ref["alpha_ins"].flatten()])
    got = _run(c)
    torch.cuda.synchronize()
    err = _errors(f"mass 0.99, r = {r:g}", got, ref, 3e-6)
    print(f"[parity-faithfulness] mass 0.99 on one position, r = {r:g}: alpha in [{float(alphas.min()):.3f}, "
          f"{float(alphas.max()):.1f}], max|err|/max|curve| = {err:.3e}")


def test_occl_curves_refuses_a_width_that_is_no_multiple_of_4():
    from dl_vqa_amd._lib import VqaHipError
    with pytest.raises(VqaHipError, match="multiple of 4"):
        _run(_case((3, 2, 2, 2, 1, 18), "shuffled"))


# ----------------------------------------------------------------------------- the whole path on the golden fixtures


@pytest.mark.parametrize("source", ["explain_occlusion", "explain", "random with ties"])
@pytest.mark.parametrize("do_option,compute_dtype", MODELS)
def test_explain_faithfulness_matches_the_brute_force_route_and_float64(do_option, compute_dtype, source):
    run = _fixture_run(do_option, compute_dtype)
    bound = _bound(compute_dtype)
    m, feats, q, ql, img = run["m"], run["feats"], run["q"], run["ql"], run["img"]
    name = f"{R.FIXTURES[do_option]} {compute_dtype} maps of {source}"
    B, n_answers = run["full"].shape
    P = feats.vn.shape[1]
    assert P == 4
    for what, given in (("arg-max", None), ("given columns", _columns(B, n_answers))):
        if source == "explain_occlusion":
            maps = m.explain_occlusion(feats, q, ql, img, answers=given).maps
        elif source == "explain":
            maps = m.explain(feats, q, ql, img, answers=given).maps
        else:
            maps = _tied_map(B, P)                                    # on the host, as [B, P]
        res = m.explain_faithfulness(feats, q, ql, img, maps, answers=given)
        torch.cuda.synchronize()
        assert isinstance(res, Faithfulness) and res.deletion.shape == res.insertion.shape == (B, P + 1)
        assert res.deletion.dtype == res.insertion.dtype == torch.float32 and res.order.dtype == res.answers.dtype == torch.int64
        assert res.order.shape == (B, P) and res.answers.shape == (B,) and res.logits.shape == (B, n_answers)
        assert not res.deletion.requires_grad and m._last_ctx is None
        assert torch.equal(res.logits, run["full"])                   # answer()'s, bit for bit
        cols = res.answers.tolist()
        assert cols == (run["full"].argmax(1).tolist() if given is None else given)
        order = FR.rank_desc(maps)
        assert torch.equal(res.order.cpu(), order)
        assert torch.equal(res.deletion[:, P], res.insertion[:, 0])
        device = _device_brute(run, order)
        brute = FR.fixture_brute_curves(do_option, cols, order)
        for curve, got, dev, want in zip(("deletion", "insertion"), (res.deletion, res.insertion), device, brute):
            _within(f"{name} {what} {curve} vs answer() on zeroed banks", got, _picked(dev, cols), bound)
            _within(f"{name} {what} {curve} vs float64 brute force", got, want, bound)
        # both ends of both curves: the full logit and the empty image
        _within(f"{name} {what} deletion[0] vs the logit", res.deletion[:, 0], _picked(run["full"], cols), bound)
        _within(f"{name} {what} insertion[P] vs the logit", res.insertion[:, P], _picked(run["full"], cols), bound)
        # the first deletion step is explain_occlusion's value of the best-ranked position
        occ = m.explain_occlusion(feats, q, ql, img, answers=cols, window=1).maps.reshape(B, P)
        _within(f"{name} {what} deletion[0] - deletion[1] vs explain_occlusion at order[0]", res.deletion[:, 0] - res.deletion[:, 1],
                occ.gather(1, res.order[:, :1])[:, 0], 2 * bound)
        # the areas
        want_auc = (brute[0][:, :-1] + brute[0][:, 1:]).sum(1) / (2 * P)
        assert res.deletion_auc().dtype == torch.float64 and res.deletion_auc().device == res.deletion.device
        assert float((res.deletion_auc().cpu() - want_auc).abs().max()) <= bound
        # the same map in its other accepted forms: bit for bit
        for form in (maps.reshape(B, *feats.grid), maps.reshape(B, P).double().cpu(), maps.reshape(B, P).to(DEV)):
            again = m.explain_faithfulness(feats, q, ql, img, form, answers=given)
            assert all(torch.equal(x, y) for x, y in zip(again, res))


@pytest.mark.parametrize("do_option,compute_dtype", MODELS)
def test_explain_faithfulness_relations(do_option, compute_dtype):
    run = _fixture_run(do_option, compute_dtype)
    bound = _bound(compute_dtype)
    m, feats, q, ql, img = run["m"], run["feats"], run["q"], run["ql"], run["img"]
    name = f"{R.FIXTURES[do_option]} {compute_dtype}"
    B, n_answers = run["full"].shape
    P = feats.vn.shape[1]
    maps = torch.randn(B, P, generator=torch.Generator().manual_seed(9))
    res = m.explain_faithfulness(feats, q, ql, img, maps)
    # a CUDA column out of range: two rows of +0.0, the other rows untouched
    bad = res.answers.clone()
    bad[2] = n_answers
    zero = m.explain_faithfulness(feats, q, ql, img, maps, answers=bad)
    for z, full in ((zero.deletion, res.deletion), (zero.insertion, res.insertion)):
        assert float(z[2].abs().max()) == 0.0 and not bool(torch.signbit(z[2]).any())
        assert torch.equal(z[:2], full[:2]) and torch.equal(z[3:], full[3:])
    # one image per chunk of U
    per_image = P * m._engine.G * m._engine.hid * 4
    chunked = m.explain_faithfulness(feats, q, ql, img, maps, _u_bytes=per_image)
    same = torch.equal(chunked.deletion, res.deletion) and torch.equal(chunked.insertion, res.insertion)
    _within(f"{name} one image per chunk vs unchunked, deletion (both curves bit-equal: {same})", chunked.deletion, res.deletion,
            bound)
    _within(f"{name} one image per chunk vs unchunked, insertion", chunked.insertion, res.insertion, bound)
    assert torch.equal(chunked.order, res.order) and torch.equal(chunked.logits, res.logits)
    # a permuted batch: the same rows, bit for bit
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(3))
    pd = perm.to(DEV)
    shuffled = m.explain_faithfulness(feats, q[pd], ql[pd], [img[i] for i in perm.tolist()], maps[perm])
    assert all(torch.equal(x, y[pd]) for x, y in zip(shuffled, res))
    # the same pairs from the two caches: whatever relation answer_pairs has to answer, the curves have it too
    qu, qlu, qidx = unique_questions(run["f"]["q"], run["f"]["q_len"])
    assert qu.shape[0] < B
    qfeats = m.encode_questions(qu.to(DEV), qlu.to(DEV))
    pairs = m.explain_faithfulness_pairs(feats, qfeats, img, qidx, maps)
    assert torch.equal(pairs.logits, m.answer_pairs(feats, qfeats, img, qidx)) and torch.equal(pairs.order, res.order)
    same = torch.equal(pairs.logits, res.logits)
    print(f"[parity-faithfulness] {name}: answer_pairs logits are answer's bit for bit: {same}")
    if same:
        assert all(torch.equal(x, y) for x, y in zip(pairs, res))
    else:
        assert float((pairs.logits - res.logits).abs().max()) <= bound
        given = m.explain_faithfulness_pairs(feats, qfeats, img, qidx, maps, answers=res.answers)
        _within(f"{name} explain_faithfulness_pairs vs explain_faithfulness, deletion", given.deletion, res.deletion, bound)
        _within(f"{name} explain_faithfulness_pairs vs explain_faithfulness, insertion", given.insertion, res.insertion, bound)
    # a float16 cache gives its widened copy's results
    if compute_dtype == "fp32":
        f16 = feats.to(torch.float16)
        f32 = f16.to(torch.float32)
        a16, a32 = m.explain_faithfulness(f16, q, ql, img, maps), m.explain_faithfulness(f32, q, ql, img, maps)
        assert all(torch.equal(x, y) for x, y in zip(a16, a32))
        p16 = m.explain_faithfulness_pairs(f16, qfeats, img, qidx, maps)
        p32 = m.explain_faithfulness_pairs(f32, qfeats, img, qidx, maps)
        assert all(torch.equal(x, y) for x, y in zip(p16, p32))
    # an empty batch
    for none in (m.explain_faithfulness(feats, q[:0], ql[:0], [], maps[:0]),
                 m.explain_faithfulness_pairs(feats, qfeats, [], [], torch.zeros(0, *feats.grid))):
        assert isinstance(none, Faithfulness) and none.deletion.shape == none.insertion.shape == (0, P + 1)
        assert none.order.shape == (0, P) and none.order.dtype == none.answers.dtype == torch.int64
        assert none.logits.shape == (0, n_answers) and none.deletion_auc().shape == (0,)
    assert m._last_ctx is None and all(p.grad is None for p in m.parameters())


def test_forward_and_backward_are_unchanged_after_explain_faithfulness():
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
    maps = torch.randn(q.shape[0], *feats.grid, generator=torch.Generator().manual_seed(4))
    got = m.explain_faithfulness(feats, q, ql, idx, maps)
    torch.cuda.synchronize()
    assert torch.equal(got.logits, m.answer(feats, q, ql, idx)) and float((got.deletion[:, 0] - got.deletion[:, -1]).abs().max()) > 1e-3
    assert m._last_ctx is None and len(m._pending) == 0
    assert m._flat_grad is flat_grad and bool((flat_grad == 3.0).all())
    assert torch.equal(torch.get_rng_state(), rng)                  # the dropout seed stream was not drawn from
    assert all(p.grad is None for p in m.parameters())
    flat_grad.zero_()
    y1, g1 = step(m)
    assert torch.equal(y1, y0)
    for k in g0:
        assert torch.equal(g1[k], g0[k]), k
    # refusals that need a device: foreign features, an index outside the cache
    with pytest.raises(RuntimeError, match="belong elsewhere"):
        fresh.explain_faithfulness(feats, q, ql, idx, maps)
    with pytest.raises(IndexError):
        m.explain_faithfulness(feats, q, ql, idx[:-1] + [feats.N], maps)
