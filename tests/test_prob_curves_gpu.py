"""GPU: probability curves and flip points -- vqa_occl_curves_hidden against float64 (tests/prob_curves_ref.py) and against
vqa_occl_curves on synthetic operands, vqa_softmax_pick against vqa_softmax_topk(k = 1) and float64, and
VqaNet.explain_faithfulness_probs / explain_faithfulness_probs_pairs on the golden fixtures against the brute-force route on the
device (answer() on per-question banks with the absent rows zeroed, then torch.softmax) and against the float64 brute force, with
the relations to answer, explain_faithfulness, a widened float16 cache, the pairs form and the three ways of chunking."""
import functools

import pytest
import torch

from dl_vqa_amd import ProbabilityCurves, unique_questions
from tests import attribution_ref as R
from tests import faithfulness_ref as FR
from tests import prob_curves_ref as PR
from tests.curves_util import MODELS, _case, _device_brute, _fixture_run, _L, _picked, _run as _run_curves, _tied_map
from tests.explain_util import build, columns as _columns, within
from tests.golden_util import Golden, tiny_cfg
from tests.test_kernels_gpu import check

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LABEL = "parity-prob-curves"
_within = functools.partial(within, label=LABEL)


def _ops():
    from dl_vqa_amd import ops
    return ops


# ----------------------------------------------------------------------------- the hidden-row walk against float64
# (B, R, gh, gw, G, hid): the grids 1 x 1, 2 x 2, 3 x 4 and 5 x 7; P = L - 1, L, L + 1 and 4 L + 1 (a second workgroup per
# question); hid of one and of several quads per lane, with and without a tail over the quads; G = 1 .. 4; B = 1 and 7
def _shapes():
    L = _L()
    return [(1, 1, 1, 1, 1, 520), (4, 3, 2, 2, 2, 1024), (1, 1, 3, 4, 3, 1028), (7, 3, 5, 7, 2, 1024), (3, 2, 5, 7, 4, 520),
            (3, 2, 5, 7, 1, 1028), (3, 2, 1, L - 1, 2, 520), (3, 2, 1, L, 3, 1024), (3, 2, 1, L + 1, 4, 1028),
            (7, 2, 1, 4 * L + 1, 2, 520)]


def _hidden(c, perm=None, order=None, out=None, U=None, slot0=0):
    d = lambda t: (t if perm is None else t[perm]).to(DEV)
    rank = c["order"] if order is None else order
    return _ops().occl_curves_hidden(d(c["base"]), (c["U"] if U is None else U).to(DEV), d(c["slot"]).to(torch.int32), d(c["probs"]),
                                     d(c["score"]), d(c["cnull"]), d(rank).to(torch.int32), slot0=slot0, out=out)


def _hidden_ref(c, order=None):
    return PR.kernel_form_hidden(c["base"], c["U"], c["slot"], c["probs"], c["score"], c["cnull"],
                                 c["order"] if order is None else order)


@pytest.mark.parametrize("index", range(10))
def test_occl_curves_hidden_matches_float64_and_the_logit_curves(index):
    shapes = _shapes()
    assert len(shapes) == 10
    shape = shapes[index]
    kind = ("shuffled", "single", "empty")[index % 3] if shape[1] > 1 else "single"
    c = _case(shape, kind)
    B, P, hid = shape[0], shape[2] * shape[3], shape[5]
    H = _hidden(c)
    torch.cuda.synchronize()
    assert H.shape == (B, 2, P + 1, hid) and H.dtype == torch.float32
    ref = _hidden_ref(c)
    check(f"occl_curves_hidden {shape} {kind}", H.double().cpu(), ref, 3e-6)
    assert float(H.min()) >= 0.0 and float(ref.max()) > 0
    # the empty image from both sides
    assert torch.equal(H[:, 0, P], H[:, 1, 0])
    # the explained column of H . W2^T + b2 (float64) is vqa_occl_curves' curve of the same operands
    deletion, insertion = _run_curves(c)
    W2, b2 = c["W2"][:, :hid].double(), c["b2"].double()
    logit = torch.einsum("bskh,bh->bsk", H.double().cpu(), W2[c["answers"]]) + b2[c["answers"]][:, None, None]
    for name, got, curve in (("deletion", logit[:, 0], deletion), ("insertion", logit[:, 1], insertion)):
        err = float((got - curve.double().cpu()).abs().max()) / float(curve.abs().max())
        print(f"[{LABEL}] occl_curves_hidden {shape} {kind}: W2[a] . H + b2[a] (float64) vs vqa_occl_curves {name}: "
              f"max|diff|/max|curve| = {err:.3e} (tol 3.0e-06)")
        assert err <= 3e-6
    # permuting the questions permutes the rows, bit for bit
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(5))
    assert torch.equal(_hidden(c, perm=perm), H[perm.to(DEV)])


def test_occl_curves_hidden_covers_a_slot_window_smaller_than_the_images_with_two_calls():
    shape = (6, 2, 5, 7, 2, 520)
    c = _case(shape, "shuffled")
    assert set(c["slot"].tolist()) == {0, 1}
    whole = _hidden(c)
    out = torch.full_like(whole, 7.0)
    for r0 in (0, 1):
        _hidden(c, U=c["U"][r0:r0 + 1], slot0=r0, out=out)
        if r0 == 0:                                                   # the other image's questions were left alone
            assert bool((out[c["slot"].to(DEV) == 1] == 7.0).all()) and bool((out[c["slot"].to(DEV) == 0] != 7.0).all())
    assert torch.equal(out, whole)


def test_an_order_entry_out_of_range_adds_nothing_to_the_hidden_rows_and_is_no_address():
    shape = (3, 2, 5, 7, 2, 520)
    c = _case(shape, "shuffled")
    order = c["order"].clone()
    order[0, 3], order[0, 20], order[1, 0], order[2, 34] = -1, 35, 2 ** 31 - 1, -(2 ** 31)
    H = _hidden(c, order=order)
    torch.cuda.synchronize()
    check("occl_curves_hidden entries out of range", H.double().cpu(), _hidden_ref(c, order), 3e-6)


def test_occl_curves_hidden_refuses_a_width_that_is_no_multiple_of_4():
    from dl_vqa_amd._lib import VqaHipError
    with pytest.raises(VqaHipError, match="multiple of 4"):
        _hidden(_case((3, 2, 2, 2, 1, 18), "shuffled"))


# ----------------------------------------------------------------------------- the probability of a given column beside top-1
def _logit_rows(rows, n_answers, seed):
    """Rows with ties, -inf entries and (row 1, when there is one) a NaN among random values spread over a few units."""
    g = torch.Generator().manual_seed(seed)
    x = 3 * torch.randn(rows, n_answers, generator=g)
    kind = torch.randint(0, 6, (rows, n_answers), generator=g)
    x = torch.where(kind == 0, torch.round(x), x)                     # ties
    x = torch.where(kind == 1, torch.full((), float("-inf")), x)
    x[:, 0] = torch.where(torch.isinf(x[:, 0]), torch.zeros(()), x[:, 0])     # no row is all -inf
    if rows > 1 and n_answers > 1:
        x[1, n_answers // 2] = float("nan")
    return x


@pytest.mark.parametrize("rows_per_question", [2, 2 * (4 + 1)])
@pytest.mark.parametrize("n_answers", [1, 7, 1000, 3003])
def test_softmax_pick_is_topk_of_one_with_the_probability_of_the_given_column(n_answers, rows_per_question):
    ops = _ops()
    questions = 3
    rows = questions * rows_per_question
    x = _logit_rows(rows, n_answers, 10 * n_answers + rows_per_question)
    padded = torch.full((rows, n_answers + 5), 9e9)                   # a padded leading dimension: the pad is never read
    padded[:, :n_answers] = x
    view = padded.to(DEV)[:, :n_answers]
    cols = torch.tensor([n_answers - 1, 0, n_answers // 2], dtype=torch.int32)
    top, top_prob, prob_at = ops.softmax_pick(view, cols.to(DEV), rows_per_question)
    idx, prob = ops.softmax_topk(view, 1)
    torch.cuda.synchronize()
    assert top.dtype == torch.int32 and top.shape == top_prob.shape == prob_at.shape == (rows,)
    assert torch.equal(top, idx[:, 0]) and torch.equal(top_prob.view(torch.int32), prob[:, 0].view(torch.int32))
    # prob_at against float64: four times what torch.softmax in fp32 loses on the same rows, and not below 1e-7
    per_row = cols.long().repeat_interleave(rows_per_question)
    want = torch.softmax(x.double(), -1).gather(1, per_row[:, None])[:, 0]
    torch_fp32 = torch.softmax(view.contiguous(), -1).gather(1, per_row.to(DEV)[:, None])[:, 0].double().cpu()
    finite = ~torch.isnan(want)
    assert bool(finite.any()) and torch.equal(torch.isnan(prob_at).cpu(), ~finite)
    torch_err = float((torch_fp32 - want)[finite].abs().max())
    tol = max(4 * torch_err, 1e-7)
    err = float((prob_at.double().cpu() - want)[finite].abs().max())
    print(f"[{LABEL}] softmax_pick A={n_answers} rows_per_question={rows_per_question}: torch.softmax fp32 vs float64 "
          f"{torch_err:.3e}, bound max(4 x that, 1e-7) = {tol:.3e}, prob_at vs float64 {err:.3e}")
    assert err <= tol
    # where the given column is the arg-max, prob_at is top_prob's bits
    same = (top.long().cpu() == per_row) & finite
    assert torch.equal(prob_at.cpu()[same], top_prob.cpu()[same])
    # a column out of range gives +0.0 and is no address; the tops do not depend on the column
    bad = torch.tensor([n_answers, -1, 2 ** 31 - 1], dtype=torch.int32)
    top2, top_prob2, zero = ops.softmax_pick(view, bad.to(DEV), rows_per_question)
    assert float(zero.abs().max()) == 0.0 and not bool(torch.signbit(zero).any())
    assert torch.equal(top2, top) and torch.equal(top_prob2.view(torch.int32), top_prob.view(torch.int32))


def test_softmax_pick_of_no_rows_and_its_refusals():
    from dl_vqa_amd._lib import VqaHipError
    ops = _ops()
    top, top_prob, prob_at = ops.softmax_pick(torch.empty(0, 24, device=DEV), torch.empty(0, dtype=torch.int32, device=DEV), 10)
    assert top.shape == top_prob.shape == prob_at.shape == (0,)
    with pytest.raises(VqaHipError, match="divide rows=6"):
        _lib_call_pick(rows=6, rpq=4)


def _lib_call_pick(rows, rpq):
    from dl_vqa_amd import _lib
    x = torch.zeros(rows, 8, device=DEV)
    cols = torch.zeros(rows, dtype=torch.int32, device=DEV)
    out = torch.zeros(3, rows, device=DEV)
    _lib.call("vqa_softmax_pick", x.data_ptr(), 8, rows, 8, cols.data_ptr(), rpq, out[0].view(torch.int32).data_ptr(),
              out[1].data_ptr(), out[2].data_ptr(), _lib.stream())


# ----------------------------------------------------------------------------- the whole path on the golden fixtures
def _soft(logits):
    return torch.softmax(logits, -1)


@functools.lru_cache(maxsize=None)
def _bounds(compute_dtype):
    """The tolerances of the whole-path tests, measured on code that is not under test (DESIGN.md 4.20's procedure): answer() on
    per-question banks with each kept set's complement zeroed, followed by torch.softmax, against the float64 brute force, over
    the three fixtures, the arg-max and the given columns, for the ranking of a fixed map with ties.  Returns (the probability
    bound, the logit bound): four times the largest absolute difference of the explained column's probability / of any logit,
    and not below 1e-7."""
    worst_p = worst_l = 0.0
    for do_option in ("+", "*", "|"):
        run = _fixture_run(do_option, compute_dtype)
        B, n_answers = run["full"].shape
        order = FR.rank_desc(_tied_map(B, run["feats"].vn.shape[1]))
        device = torch.stack(_device_brute(run, order), 1)            # [B, 2, P+1, A]
        want = PR.fixture_brute_logit_curves(do_option, order)
        worst_l = max(worst_l, float((device.double().cpu() - want).abs().max()))
        for cols in (run["full"].argmax(1).tolist(), _columns(B, n_answers)):
            ref = PR.curve_stats(want, cols)["prob"]
            worst_p = max(worst_p, float((_picked(_soft(device), cols).double().cpu() - ref).abs().max()))
    bound_p, bound_l = max(4 * worst_p, 1e-7), max(4 * worst_l, 1e-7)
    print(f"[{LABEL}] {compute_dtype}: answer() on zeroed banks + torch.softmax vs float64 brute force over the three fixtures: "
          f"probability max|diff| = {worst_p:.3e}, bound max(4 x that, 1e-7) = {bound_p:.3e}; logits max|diff| = {worst_l:.3e}, "
          f"logit bound = {bound_l:.3e}")
    return bound_p, bound_l


def _check_tops(tag, res, ref, logit_bound, bound):
    """The cap rule: an entry is compared where the float64 margin exceeds four times the logit bound; at most 5 % are not."""
    mask, left_out = PR.comparable(ref["margin"], logit_bound)
    got_top = torch.stack([res.deletion_top, res.insertion_top], 1).long().cpu()
    got_prob = torch.stack([res.deletion_top_prob, res.insertion_top_prob], 1).double().cpu()
    agree = float((got_top == ref["top"]).double().mean())
    print(f"[{LABEL}] {tag} tops: share of (b, k) entries left out of the comparison {left_out:.4f} (cap {PR.MAX_LEFT_OUT}), "
          f"agreement over all entries {agree:.4f}")
    assert left_out <= PR.MAX_LEFT_OUT
    assert torch.equal(got_top[mask], ref["top"][mask])
    err = float((got_prob - ref["top_prob"])[mask].abs().max())
    assert err <= bound, f"{tag}: top probability {err} > {bound}"


@pytest.mark.parametrize("source", ["explain_occlusion", "explain", "random with ties"])
@pytest.mark.parametrize("do_option,compute_dtype", MODELS)
def test_explain_faithfulness_probs_matches_the_brute_force_route_and_float64(do_option, compute_dtype, source):
    run = _fixture_run(do_option, compute_dtype)
    bound, logit_bound = _bounds(compute_dtype)
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
        res = m.explain_faithfulness_probs(feats, q, ql, img, maps, answers=given)
        torch.cuda.synchronize()
        assert isinstance(res, ProbabilityCurves)
        for field in ("deletion", "insertion", "deletion_top_prob", "insertion_top_prob"):
            assert getattr(res, field).shape == (B, P + 1) and getattr(res, field).dtype == torch.float32
        for field in ("deletion_top", "insertion_top"):
            assert getattr(res, field).shape == (B, P + 1) and getattr(res, field).dtype == torch.int32
        assert res.order.dtype == res.answers.dtype == torch.int64 and res.order.shape == (B, P) and res.answers.shape == (B,)
        assert not res.deletion.requires_grad and m._last_ctx is None
        logit_curves = m.explain_faithfulness(feats, q, ql, img, maps, answers=given)
        assert torch.equal(res.logits, run["full"]) and torch.equal(res.order, logit_curves.order)    # bit for bit
        assert torch.equal(res.answers, logit_curves.answers)
        cols = res.answers.tolist()
        assert cols == (run["full"].argmax(1).tolist() if given is None else given)
        order = FR.rank_desc(maps)
        assert torch.equal(res.order.cpu(), order)
        assert torch.equal(res.deletion[:, P], res.insertion[:, 0]) and torch.equal(res.deletion_top[:, P], res.insertion_top[:, 0])
        device = _soft(torch.stack(_device_brute(run, order), 1))     # [B, 2, P+1, A]
        ref = PR.curve_stats(PR.fixture_brute_logit_curves(do_option, order), cols)
        for side, curve, got in ((0, "deletion", res.deletion), (1, "insertion", res.insertion)):
            _within(f"{name} {what} {curve} vs answer() on zeroed banks + softmax", got, _picked(device[:, side], cols), bound)
            _within(f"{name} {what} {curve} vs float64 brute force", got, ref["prob"][:, side], bound)
        # both ends of both curves: the probability of the column on the full image
        full = _picked(_soft(run["full"]), cols)
        _within(f"{name} {what} deletion[0] vs softmax(logits)", res.deletion[:, 0], full, bound)
        _within(f"{name} {what} insertion[P] vs softmax(logits)", res.insertion[:, P], full, bound)
        _check_tops(f"{name} {what}", res, ref, logit_bound, bound)
        # the areas and the flip points
        want_auc = (ref["prob"][:, 0, :-1] + ref["prob"][:, 0, 1:]).sum(1) / (2 * P)
        assert res.deletion_auc().dtype == torch.float64 and res.deletion_auc().device == res.deletion.device
        assert float((res.deletion_auc().cpu() - want_auc).abs().max()) <= bound
        flips = (res.deletion_flip(), res.insertion_flip())
        assert all(f.dtype == torch.int64 and f.shape == (B,) and f.device == res.deletion.device for f in flips)
        for b in range(B):
            gone = [k for k in range(P + 1) if int(res.deletion_top[b, k]) != cols[b]]
            back = [k for k in range(P + 1) if int(res.insertion_top[b, k]) == cols[b]]
            assert int(flips[0][b]) == (gone[0] if gone else P + 1) and int(flips[1][b]) == (back[0] if back else P + 1)
        if given is None:                                             # the arg-max of the full image is the explained column
            assert bool((res.deletion_flip() > 0).all()) and bool((res.insertion_flip() <= P).all())
        # the same map in its other accepted forms: bit for bit
        for form in (maps.reshape(B, *feats.grid), maps.reshape(B, P).double().cpu(), maps.reshape(B, P).to(DEV)):
            again = m.explain_faithfulness_probs(feats, q, ql, img, form, answers=given)
            assert all(torch.equal(x, y) for x, y in zip(again, res))


def _close(tag, got, res, bound):
    """Two results of the same pairs under another chunking: the curves to the bound (the product with lin2 may pick its tiles
    by the row count), the rest bit for bit; says whether everything came out bit-equal."""
    same = all(torch.equal(x, y) for x, y in zip(got, res))
    print(f"[{LABEL}] {tag}: bit-equal to the unchunked call: {same}")
    for field in ("deletion", "insertion", "deletion_top_prob", "insertion_top_prob"):
        _within(f"{tag} {field}", getattr(got, field), getattr(res, field), bound)
    assert torch.equal(got.order, res.order) and torch.equal(got.logits, res.logits) and torch.equal(got.answers, res.answers)


@pytest.mark.parametrize("do_option,compute_dtype", MODELS)
def test_explain_faithfulness_probs_relations(do_option, compute_dtype):
    run = _fixture_run(do_option, compute_dtype)
    bound, _ = _bounds(compute_dtype)
    m, feats, q, ql, img = run["m"], run["feats"], run["q"], run["ql"], run["img"]
    eng = m._engine
    name = f"{R.FIXTURES[do_option]} {compute_dtype}"
    B, n_answers = run["full"].shape
    P = feats.vn.shape[1]
    maps = torch.randn(B, P, generator=torch.Generator().manual_seed(9))
    res = m.explain_faithfulness_probs(feats, q, ql, img, maps)
    # a CUDA column out of range: two probability rows of +0.0, the tops and the other rows untouched
    bad = res.answers.clone()
    bad[2] = n_answers
    zero = m.explain_faithfulness_probs(feats, q, ql, img, maps, answers=bad)
    for z, full in ((zero.deletion, res.deletion), (zero.insertion, res.insertion)):
        assert float(z[2].abs().max()) == 0.0 and not bool(torch.signbit(z[2]).any())
        assert torch.equal(z[:2], full[:2]) and torch.equal(z[3:], full[3:])
    assert torch.equal(zero.deletion_top, res.deletion_top) and torch.equal(zero.insertion_top_prob, res.insertion_top_prob)
    # chunk invariance, three ways: one image per chunk of U, one question per sub-chunk, a permuted batch
    per_image = P * eng.G * eng.hid * 4
    _close(f"{name} one image per chunk of U", m.explain_faithfulness_probs(feats, q, ql, img, maps, _u_bytes=per_image), res, bound)
    assert eng.prob_curve_questions(P, 1) == 1 and eng.prob_curve_questions(P) >= B
    _close(f"{name} one question per sub-chunk", m.explain_faithfulness_probs(feats, q, ql, img, maps, _ws_bytes=1), res, bound)
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(3))
    pd = perm.to(DEV)
    shuffled = m.explain_faithfulness_probs(feats, q[pd], ql[pd], [img[i] for i in perm.tolist()], maps[perm])
    _close(f"{name} a permuted batch", shuffled, ProbabilityCurves(*(t[pd] for t in res)), bound)
    # the same pairs from the two caches: whatever relation answer_pairs has to answer, the curves have it too
    qu, qlu, qidx = unique_questions(run["f"]["q"], run["f"]["q_len"])
    qfeats = m.encode_questions(qu.to(DEV), qlu.to(DEV))
    pairs = m.explain_faithfulness_probs_pairs(feats, qfeats, img, qidx, maps)
    assert torch.equal(pairs.logits, m.answer_pairs(feats, qfeats, img, qidx)) and torch.equal(pairs.order, res.order)
    same = torch.equal(pairs.logits, res.logits)
    print(f"[{LABEL}] {name}: answer_pairs logits are answer's bit for bit: {same}")
    if same:
        assert all(torch.equal(x, y) for x, y in zip(pairs, res))
    else:
        given = m.explain_faithfulness_probs_pairs(feats, qfeats, img, qidx, maps, answers=res.answers)
        _within(f"{name} pairs vs plain, deletion", given.deletion, res.deletion, bound)
        _within(f"{name} pairs vs plain, insertion", given.insertion, res.insertion, bound)
    # a float16 cache gives its widened copy's results
    if compute_dtype == "fp32":
        f16 = feats.to(torch.float16)
        f32 = f16.to(torch.float32)
        a16, a32 = m.explain_faithfulness_probs(f16, q, ql, img, maps), m.explain_faithfulness_probs(f32, q, ql, img, maps)
        assert all(torch.equal(x, y) for x, y in zip(a16, a32))
        p16 = m.explain_faithfulness_probs_pairs(f16, qfeats, img, qidx, maps)
        p32 = m.explain_faithfulness_probs_pairs(f32, qfeats, img, qidx, maps)
        assert all(torch.equal(x, y) for x, y in zip(p16, p32))
    # an empty batch
    for none in (m.explain_faithfulness_probs(feats, q[:0], ql[:0], [], maps[:0]),
                 m.explain_faithfulness_probs_pairs(feats, qfeats, [], [], torch.zeros(0, *feats.grid))):
        assert isinstance(none, ProbabilityCurves) and none.deletion.shape == none.insertion_top.shape == (0, P + 1)
        assert none.deletion_top.dtype == torch.int32 and none.order.shape == (0, P) and none.order.dtype == torch.int64
        assert none.logits.shape == (0, n_answers) and none.deletion_auc().shape == none.insertion_flip().shape == (0,)
    assert m._last_ctx is None and all(p.grad is None for p in m.parameters())


def test_forward_and_backward_are_unchanged_after_explain_faithfulness_probs():
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
    got = m.explain_faithfulness_probs(feats, q, ql, idx, maps)
    torch.cuda.synchronize()
    assert torch.equal(got.logits, m.answer(feats, q, ql, idx))
    assert float((got.deletion.sum() + got.insertion.sum())) > 0 and float(got.deletion.max()) <= 1.0
    assert m._last_ctx is None and len(m._pending) == 0
    assert m._flat_grad is flat_grad and bool((flat_grad == 3.0).all())
    assert torch.equal(torch.get_rng_state(), rng)                  # the dropout seed stream was not drawn from
    assert all(p.grad is None for p in m.parameters())
    flat_grad.zero_()
    y1, g1 = step(m)
    assert torch.equal(y1, y0)
    for k in g0:
        assert torch.equal(g1[k], g0[k]), k
    with pytest.raises(RuntimeError, match="belong elsewhere"):
        fresh.explain_faithfulness_probs(feats, q, ql, idx, maps)
