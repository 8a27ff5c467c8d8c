"""GPU: training through shared image features -- the three attention-stage kernels against float64 evaluations of the
formulas in include/vqa_hip.h, and VqaNet.forward_shared / train.run_batch_shared against the CPU oracle run on the
GATHERED inputs v[image_index] (autograd then sums the image-side gradients over an image's questions by itself).  In train
mode the oracle gets the masks the HIP path applies, extracted as data: one row per IMAGE for the image-side sites, gathered
by image_index; one row per question for the others (tests/hip_masks.py)."""
import pytest
import torch

from dl_vqa_amd import group_by_image
from tests.golden_util import TINY_CASES, Golden, full_cfg, full_inputs, tiny_cfg
from tests.test_kernels_gpu import check
from tests.test_model_gpu import ZERO_GRAD, build, grad_err, rel
from tests.test_multi_question_gpu import _grouping, score_reference

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

SHAPES = [(3, 7, 4, 24, 2), (2, 9, 676, 1024, 2), (5, 5, 169, 256, 1), (3, 6, 100, 520, 4), (2, 5, 37, 2048, 3)]
SEED_X = 0x1234ABCD5678


def _ops():
    from dl_vqa_amd import ops
    return ops


def _score_inputs(N, B, P, mid, G, mode, kind):
    g = torch.Generator().manual_seed(N * 1000 + B * 10 + mode)
    vp = torch.randn(N * P, mid, generator=g)
    qp = torch.randn(B, mid, generator=g)
    wx = torch.randn(G, 2 * mid if mode == 2 else mid, generator=g)
    bx = torch.randn(G, generator=g)
    img = _grouping(kind, N, B, g)
    dscore = torch.randn(B, G, P, generator=g)
    return vp, qp, wx, bx, img, dscore


def _x_mask(B, P, xld, p):
    """The keep-scale mask of the x dropout as data: vqa_dropout on ones of the logical tensor [B, P, xld]."""
    if p == 0:
        return None
    m = _ops().dropout(torch.ones(B, P, xld, device=DEV), p, SEED_X).cpu()
    vals = set(round(float(x), 4) for x in m.unique())
    assert vals == {0.0, round(1 / (1 - p), 4)}
    return m.double()


def masked_score(vp, qp, wx, bx, img, P, mode, mask):
    """float64: score[b][g][p] = bx[g] + sum_m wx[g][m] * mask[b][p][m] * x[b][p][m], x as in include/vqa_hip.h."""
    N, mid = vp.shape[0] // P, vp.shape[1]
    v = vp.view(N, P, mid)[img]                                   # [B, P, mid]
    q = qp[:, None, :]
    if mode == 0:
        x = torch.relu(v + q)
    elif mode == 1:
        x = torch.relu(v * q)
    else:
        x = torch.cat([torch.relu(v), torch.relu(q).expand(-1, P, -1)], dim=2)
    if mask is not None:
        x = x * mask
    return (x @ wx.t() + bx).permute(0, 2, 1)


# ----------------------------------------------------------------------------- kernels 1 and 3
@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("kind", ["empty", "single", "shuffled"])
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("N,B,P,mid,G", SHAPES)
def test_grouped_score_fwd_bwd_match_float64(N, B, P, mid, G, mode, kind, p):
    """Every element of the scores and of the three gradients against float64.  Scores: the 3e-6 of the grouped forward
    test (measured worst case over the 90 cases on an MI355X: 1.8e-7).  Gradients: the 1e-5 tests/test_kernels_gpu.py applies
    to att_score_bwd.  The grouped sums are longer than the 27 terms that test covers (dq': up to 676 positions; dwx: up to
    9 x 676 = 6084 terms; dvprime: up to 9 questions), so the error was measured against float64 on an MI355X: worst case
    over the 90 cases dvprime 1.3e-7, dq' 2.6e-7, dwx 3.9e-7 of the largest entry.  1e-5 is 26 x the observed worst case and
    is kept as the bound."""
    ops = _ops()
    vp, qp, wx, bx, img, dscore = _score_inputs(N, B, P, mid, G, mode, kind)
    order, offsets = group_by_image(img, N)
    mask = _x_mask(B, P, wx.shape[1], p)
    vr, qr, wr = (t.double().requires_grad_(True) for t in (vp, qp, wx))
    want = masked_score(vr, qr, wr, bx.double(), img, P, mode, mask)
    (want * dscore.double()).sum().backward()
    if p == 0:
        assert float((want.detach() - score_reference(vp, qp, wx, bx, img, P, mode)).abs().max()) < 1e-12

    d = lambda t: t.to(DEV)
    args = (d(vp), d(qp), d(wx), d(bx), d(order), d(offsets), N, B, P, mode)
    score = ops.att_score_grouped_drop_fwd(*args, p, SEED_X)
    dvp, dq_part, dwx_part, NT = ops.att_score_grouped_bwd(d(dscore), d(vp), d(qp), d(wx), d(order), d(offsets), N, B, P, mode, p,
                                                           SEED_X)
    dq = torch.empty(B, mid, device=DEV)
    ops.sum_parts(dq_part, dq, B, NT, mid)
    dwx = torch.empty(wx.numel(), device=DEV)
    ops.colsum(dwx_part, N * NT, wx.numel(), dwx)
    torch.cuda.synchronize()
    tag = f"{N,B,P,mid,G} mode {mode} {kind} p {p}"
    check(f"att_score_grouped_drop {tag}", score, want.detach(), 3e-6)
    check(f"att_score_grouped_bwd dvprime {tag}", dvp, vr.grad, 1e-5)
    check(f"att_score_grouped_bwd dq' {tag}", dq, qr.grad, 1e-5)
    check(f"att_score_grouped_bwd dwx {tag}", dwx.view_as(wx), wr.grad, 1e-5)
    # rows of images nobody asks about: exactly zero, and written
    asked = set(img.tolist())
    for n in range(N):
        if n not in asked:
            assert float(dvp.view(N, P, mid)[n].abs().max()) == 0.0, n
    if p == 0:                                                     # the inference entry point's device code, bit for bit
        assert torch.equal(score, ops.att_score_grouped_fwd(*args))
    # the same call twice: the same bits
    score2 = ops.att_score_grouped_drop_fwd(*args, p, SEED_X)
    dvp2, dq_part2, dwx_part2, _ = ops.att_score_grouped_bwd(d(dscore), d(vp), d(qp), d(wx), d(order), d(offsets), N, B, P, mode,
                                                             p, SEED_X)
    torch.cuda.synchronize()
    assert torch.equal(score, score2) and torch.equal(dvp, dvp2)
    assert torch.equal(dq_part, dq_part2) and torch.equal(dwx_part, dwx_part2)


# ----------------------------------------------------------------------------- kernel 2
@pytest.mark.parametrize("kind", ["empty", "single", "shuffled"])
@pytest.mark.parametrize("N,B,P,C,G", [(2, 7, 676, 256, 2), (3, 7, 70, 132, 3), (3, 9, 100, 72, 1), (4, 11, 17, 64, 4),
                                       (2, 5, 65, 8, 2)])
def test_apply_gather_bwd_matches_float64(N, B, P, C, G, kind):
    """dscore, its row sums and the per-image weighted-sum branch of d loss / d vn against float64, with the bound
    tests/test_kernels_gpu.py applies to att_apply_bwd (1e-5).  The per-image sum adds at most B x G = 44 terms per element,
    more than the 2 that test covers; measured worst case over the 15 cases on an MI355X: dscore 2.6e-7, dvn 2.6e-7 of the
    largest entry -- 1e-5 is 39 x that and is kept."""
    ops = _ops()
    g = torch.Generator().manual_seed(B * 1000 + P + C)
    vn = torch.randn(N, P, C, generator=g)
    pr = torch.softmax(torch.randn(B, G, P, generator=g) * 2, dim=-1)
    ld = G * C + 12
    dout = torch.randn(B, ld, generator=g)
    img = _grouping(kind, N, B, g)
    order, offsets = group_by_image(img, N)
    do = dout[:, :G * C].double().view(B, G, C)
    dprob = torch.einsum("bpc,bgc->bgp", vn.double()[img], do)
    prd = pr.double()
    ds_ref = prd * (dprob - (prd * dprob).sum(-1, keepdim=True))
    dvn_ref = torch.zeros(N, P, C, dtype=torch.float64).index_add_(0, img, torch.einsum("bgp,bgc->bpc", prd, do))
    rows = torch.full((B, G), 7.0, device=DEV)
    d = lambda t: t.to(DEV)
    dscore, dvn = ops.att_apply_gather_bwd(d(dout), ld, d(pr), d(vn), d(img.to(torch.int32)), d(order), d(offsets), rowsum=rows)
    dscore2, dvn2 = ops.att_apply_gather_bwd(d(dout), ld, d(pr), d(vn), d(img.to(torch.int32)), d(order), d(offsets))
    torch.cuda.synchronize()
    tag = f"{N,B,P,C,G} {kind}"
    check(f"att_apply_gather_bwd dscore {tag}", dscore, ds_ref, 1e-5)
    check(f"att_apply_gather_bwd dvn {tag}", dvn, dvn_ref, 1e-5)
    assert float((rows.double().cpu() - ds_ref.sum(-1)).abs().max()) < 1e-5      # ~0: softmax gradients sum to zero
    asked = set(img.tolist())
    for n in range(N):
        if n not in asked:
            assert float(dvn[n].abs().max()) == 0.0, n
    assert torch.equal(dscore, dscore2) and torch.equal(dvn, dvn2)


def test_apply_bwd_keeps_its_bits_and_the_gather_form_equals_it_at_arange():
    """vqa_att_apply_bwd runs the (sample, image) row body the gather kernel runs: with one question per image, in order,
    both give the same bits -- dscore, row sums and dvn; and dvn = NULL (what the train step passes) changes nothing else."""
    ops = _ops()
    g = torch.Generator().manual_seed(5)
    B, P, C, G = 5, 169, 72, 2
    ld = G * C + 8
    vn, dout = torch.randn(B, P, C, generator=g).to(DEV), torch.randn(B, ld, generator=g).to(DEV)
    pr = torch.softmax(torch.randn(B, G, P, generator=g), dim=-1).to(DEV)
    r0, r1 = torch.zeros(B, G, device=DEV), torch.zeros(B, G, device=DEV)
    ds0, dvn0 = ops.att_apply_bwd(dout, ld, pr, vn, rowsum=r0)
    ds_n, none = ops.att_apply_bwd(dout, ld, pr, vn, want_dvn=False)
    order, offsets = group_by_image(torch.arange(B), B)
    ds1, dvn1 = ops.att_apply_gather_bwd(dout, ld, pr, vn, torch.arange(B, dtype=torch.int32, device=DEV), order.to(DEV),
                                          offsets.to(DEV), rowsum=r1)
    torch.cuda.synchronize()
    assert none is None and torch.equal(ds_n, ds0)
    assert torch.equal(ds1, ds0) and torch.equal(dvn1, dvn0) and torch.equal(r1, r0)
    # against float64, with test_kernels_gpu's bound for this kernel
    do = dout[:, :G * C].double().cpu().view(B, G, C)
    check("att_apply_bwd dvn", dvn0, torch.einsum("bgp,bgc->bpc", pr.double().cpu(), do), 1e-5)


# ----------------------------------------------------------------------------- the whole path
IMAGE_INDEX = torch.tensor([0, 1, 2, 2, 0, 1, 1])
QSEL = torch.tensor([0, 1, 2, 0, 1, 2, 1])


def oracle_shared(sd, cfg, v, q, ql, a_idx, a_val, image_index, masks=None):
    """The existing oracle on the gathered images; the image gradient w.r.t. the UNIQUE images comes from the same oracle
    forward differentiated through the gather (autograd sums the questions of an image)."""
    from oracle import vqa_oracle as O
    y, loss, grads = O.loss_and_grads(sd, cfg, v[image_index], q, ql, a_idx, a_val, masks=masks)
    vu = v.clone().requires_grad_(True)
    logits = O.vqa_forward(sd, cfg, vu[image_index], q, ql, masks=masks)
    dv, = torch.autograd.grad(O.soft_ce_loss(logits, a_idx, a_val), vu)
    return y, loss, grads, dv


def shared_step(m, v, q, ql, a_idx, a_val, image_index, want_dv=True):
    from dl_vqa_amd.train import soft_ce_loss_and_score
    for p in m.parameters():
        p.grad = None
    vd = v.to(DEV).requires_grad_(want_dv)
    y = m.forward_shared(vd, q.to(DEV), ql.to(DEV), image_index)
    loss, _ = soft_ce_loss_and_score(y, a_idx.to(DEV), a_val.to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    return y.detach(), loss.detach(), {k: p.grad.clone() for k, p in m.named_parameters()}, vd.grad


def _fixture_batch(g):
    return g.t["v"][:3], g.t["q"][QSEL], g.t["q_len"][QSEL], g.t["a_idx"][QSEL], g.t["a_val"][QSEL]


@pytest.mark.parametrize("name", TINY_CASES)
def test_forward_shared_matches_oracle_on_fixtures(name):
    """Eval mode, 3 images, 7 questions: logits, loss, every parameter gradient and the image gradient against the oracle
    on v[image_index], with the tolerances tests/test_model_gpu.py applies to forward / backward on these fixtures."""
    g = Golden(name)
    cfg = tiny_cfg(g.meta)
    m = build(cfg, g.meta["V"], g.sd).eval()
    v, q, ql, a_idx, a_val = _fixture_batch(g)
    y_ref, loss_ref, g_ref, dv_ref = oracle_shared(g.sd, cfg, v, q, ql, a_idx, a_val, IMAGE_INDEX)
    y, loss, grads, dv = shared_step(m, v, q, ql, a_idx, a_val, IMAGE_INDEX)
    err = float((y.cpu() - y_ref).abs().max())
    print(f"[shared] {name}: logits max abs err {err:.3e}; loss {float(loss):.6f} vs {float(loss_ref):.6f}")
    assert y.shape == (7, cfg["max_answers"]) and err < 1e-5
    assert abs(float(loss) - float(loss_ref)) < 1e-5
    for k in grads:
        e = grad_err(k, grads[k], g_ref[k], g.meta["do_option"])
        print(f"[shared] {name} grad {k}: {e:.3e}")
        assert e < 2e-4, (k, e)
    e = rel(dv, dv_ref)
    print(f"[shared] {name} image grad: {e:.3e}")
    assert dv.shape == v.shape and e <= 2e-4
    assert m._last_backward_direct is True
    # outside a grad context: the same logits, nothing kept
    m._last_ctx = None
    with torch.no_grad():
        y_ng = m.forward_shared(v.to(DEV), q.to(DEV), ql.to(DEV), IMAGE_INDEX.tolist())
    assert torch.equal(y_ng, y) and m._last_ctx is None and len(m._pending) == 0
    # additional check, not the judge: one question per image agrees with forward / backward on the same batch
    from dl_vqa_amd.train import soft_ce_loss_and_score
    vf, qf, qlf = g.t["v"], g.t["q"], g.t["q_len"]
    y_s, _, g_s, dv_s = shared_step(m, vf, qf, qlf, g.t["a_idx"], g.t["a_val"], torch.arange(vf.shape[0]))
    for p in m.parameters():
        p.grad = None
    vd = vf.to(DEV).requires_grad_(True)
    y_f = m(vd, qf.to(DEV), qlf.to(DEV))
    soft_ce_loss_and_score(y_f, g.t["a_idx"].to(DEV), g.t["a_val"].to(DEV))[0].backward()
    torch.cuda.synchronize()
    assert float((y_s - y_f.detach()).abs().max()) < 1e-5
    for k, p in m.named_parameters():
        assert grad_err(k, g_s[k], p.grad, g.meta["do_option"]) < 2e-4, k
    assert rel(dv_s, vd.grad) <= 2e-4


def shared_masks(m, ctx, image_index, T):
    """Image-side sites: one row per image, gathered by image_index; question-side sites: one row per question."""
    from tests.hip_masks import hip_masks
    g = ctx.acts[-1].shape[1]
    per_image = hip_masks(m._engine, ctx.seed, ctx.N, T, g, DEV)
    masks = hip_masks(m._engine, ctx.seed, ctx.B, T, g, DEV)
    for site in ("image", "att_v"):
        masks[site] = per_image[site][image_index]
    return masks


@pytest.mark.parametrize("do_option", ["+", "*", "|"])
def test_forward_shared_train_mode_matches_oracle_with_shared_masks(do_option):
    """Train mode, all 7 dropout sites at p = 0.3 (the configuration of the *_train fixtures), weights of the fixture: the
    masks the HIP path applies go to the oracle as data.  A wrong index convention of the x mask in the grouped forward or
    backward kernel (image instead of question, another row length) fails here.  Tolerances of
    test_model_gpu.test_train_mode_matches_oracle_with_shared_masks."""
    from oracle import vqa_oracle as O
    g = Golden({"+": "tiny_plus", "*": "tiny_mul", "|": "tiny_cat"}[do_option])
    cfg = tiny_cfg(g.meta)
    m = build(cfg, g.meta["V"], g.sd).train()
    v, q, ql, a_idx, a_val = _fixture_batch(g)
    torch.manual_seed(123)
    rng = torch.get_rng_state()
    y, loss, grads, dv = shared_step(m, v, q, ql, a_idx, a_val, IMAGE_INDEX)
    ctx = m._last_ctx
    assert ctx.p_att == 0.3 and ctx.seed != 0 and (ctx.N, ctx.B) == (3, 7)
    torch.set_rng_state(rng)
    assert ctx.seed == m._next_seed()                                 # one draw per training forward
    masks = shared_masks(m, ctx, IMAGE_INDEX, q.shape[1])
    for k, mk in masks.items():
        vals = set(round(float(x), 4) for x in mk.unique())
        assert vals == {0.0, round(1 / 0.7, 4)}, (k, vals)
        assert mk.shape[0] == 7, k
    y_ref, loss_ref, g_ref, dv_ref = oracle_shared(g.sd, cfg, v, q, ql, a_idx, a_val, IMAGE_INDEX, masks=masks)
    err = float((y.cpu() - y_ref).abs().max())
    print(f"[shared] train-mode ({do_option}) logits max abs err {err:.3e}; loss {float(loss):.6f} vs {float(loss_ref):.6f}")
    assert err < 2e-5
    assert abs(float(loss) - float(loss_ref)) < 1e-5
    assert float((y_ref - O.vqa_forward(g.sd, cfg, v[IMAGE_INDEX], q, ql)).abs().max()) > 1e-2     # the masks matter
    for k in grads:
        e = grad_err(k, grads[k], g_ref[k], "+")
        print(f"[shared] train-mode ({do_option}) grad {k}: {e:.3e}")
        assert e < 2e-4, (k, e)
    e = rel(dv, dv_ref)
    print(f"[shared] train-mode ({do_option}) image grad: {e:.3e}")
    assert e <= 2e-4
    # eval mode draws nothing
    m.eval()
    rng = torch.get_rng_state()
    with torch.no_grad():
        m.forward_shared(v.to(DEV), q.to(DEV), ql.to(DEV), IMAGE_INDEX)
    assert torch.equal(torch.get_rng_state(), rng)


def _full224_case():
    from dl_vqa_amd import VqaNet
    g = Golden("full224_seed1")
    meta = g.meta
    cfg = full_cfg(meta["A"])
    v, q, ql, a_idx, a_val, _ = full_inputs(meta)
    image_index, qsel = torch.tensor([0, 1, 1, 0]), torch.tensor([0, 1, 0, 1])
    return meta, cfg, (v, q[qsel], ql[qsel], a_idx[qsel], a_val[qsel]), image_index


@pytest.mark.parametrize("compute_dtype", ["fp32", "fp32x3"])
def test_forward_shared_full224_matches_oracle(compute_dtype):
    """North-star architecture at 224 x 224, 2 images, 4 questions (image_index [0, 1, 1, 0]) against the oracle, in the
    mode and with the tolerances of the existing full224 test against the oracle
    (test_model_gpu.test_train_mode_full224_matches_oracle_with_shared_masks): train mode, the HIP masks given to the oracle
    as data, logits 1e-3, loss 1e-4, every gradient element 1e-3 of the largest.  The oracle runs in float64.

    Eval mode at the initial weights cannot judge the attention gradients at these tolerances, whatever the path: the
    gradients of v_conv.weight, q_lin.weight and q_lin.bias are ~1e-7 there, sums over positions of terms that cancel
    (softmax gradients sum to zero over positions and the features barely vary), and fp32 rounding upstream leaves 1.09e-2,
    1.11e-2 and 1.01e-2 of the largest entry against the float64 oracle -- measured on an MI355X for forward_shared AND for
    model(v[image_index], q, q_len) on this batch, the two agreeing to 3.5e-6.  So in eval mode the logits and the loss are
    held to the oracle and every gradient to the one-image-per-question path (an additional check, not the judge)."""
    from oracle import vqa_oracle as O
    from dl_vqa_amd.train import soft_ce_loss_and_score
    meta, cfg, batch, image_index = _full224_case()
    v, q, ql, a_idx, a_val = batch
    torch.manual_seed(meta["seed"])
    m = build(cfg, meta["V"], compute_dtype=compute_dtype).train()
    sd64 = {k: t.detach().cpu().double() for k, t in m.state_dict().items()}
    y, loss, grads, _ = shared_step(m, *batch, image_index, want_dv=False)
    ctx = m._last_ctx
    masks = shared_masks(m, ctx, image_index, q.shape[1])
    y_ref, loss_ref, g_ref = O.loss_and_grads(sd64, cfg, v.double()[image_index], q, ql, a_idx, a_val, masks=masks)
    err = float((y.cpu().double() - y_ref).abs().max())
    print(f"[shared] full224 train ({compute_dtype}) logits max abs err {err:.3e}; loss {float(loss):.6f} vs {float(loss_ref):.6f}")
    assert err < 1e-3
    assert abs(float(loss) - float(loss_ref)) < 1e-4
    for k in grads:
        e = grad_err(k, grads[k], g_ref[k], "+")
        print(f"[shared] full224 train ({compute_dtype}) grad {k}: {e:.3e}")
        assert e < 1e-3, (k, e)
    # ---- eval mode
    m.eval()
    y_ref, loss_ref, g_ref = O.loss_and_grads(sd64, cfg, v.double()[image_index], q, ql, a_idx, a_val)
    y, loss, grads, _ = shared_step(m, *batch, image_index, want_dv=False)
    assert float((y.cpu().double() - y_ref).abs().max()) < 1e-3
    assert abs(float(loss) - float(loss_ref)) < 1e-4
    for p in m.parameters():
        p.grad = None
    y_f = m(v[image_index].to(DEV), q.to(DEV), ql.to(DEV))
    soft_ce_loss_and_score(y_f, a_idx.to(DEV), a_val.to(DEV))[0].backward()
    torch.cuda.synchronize()
    for k, p in m.named_parameters():
        e_or, e_fw = grad_err(k, grads[k], g_ref[k], "+"), grad_err(k, grads[k], p.grad, "+")
        print(f"[shared] full224 eval ({compute_dtype}) grad {k}: vs oracle {e_or:.3e}, vs forward {e_fw:.3e}")
        assert e_fw < 1e-3, (k, e_fw)


def test_fused_adam_step_after_run_batch_shared_matches_oracle():
    from oracle import vqa_oracle as O
    from dl_vqa_amd.train import FusedAdam, run_batch_shared
    g = Golden("tiny_plus")
    cfg = tiny_cfg(g.meta)
    m = build(cfg, g.meta["V"], g.sd).eval()
    v, q, ql, a_idx, a_val = _fixture_batch(g)
    _, loss_ref, g_ref = O.loss_and_grads(g.sd, cfg, v[IMAGE_INDEX], q, ql, a_idx, a_val)
    batch = (v, q, a_idx, a_val, g.t["a_len"][QSEL], torch.arange(7), ql)
    opt = FusedAdam(m, lr=5e-4)
    loss, score = run_batch_shared(m, batch, 12, IMAGE_INDEX)
    opt.zero_grad()
    loss.backward()
    assert abs(float(loss) - float(loss_ref)) < 1e-5                  # divided by the 7 questions, as the oracle divides
    assert m._last_backward_direct is True
    for k, p in m.named_parameters():                                 # p.grad are views of the flat buffer
        o, n = m._offsets[k]
        assert p.grad.data_ptr() == m._flat_grad.data_ptr() + 4 * o, k
    opt.step()
    torch.cuda.synchronize()
    for k, p in m.named_parameters():
        if k == ZERO_GRAD:
            continue
        ref = g.sd[k].clone()
        O.adam_step(ref, g_ref[k], torch.zeros_like(ref), torch.zeros_like(ref), 1, 5e-4)
        upd, upd_ref = p.detach().cpu() - g.sd[k], ref - g.sd[k]
        big = g_ref[k].abs() > 1e-3 * g_ref[k].abs().max()
        if bool(big.any()):
            assert float((upd - upd_ref)[big].abs().max()) < 1e-2 * 5e-4, k
    # a second backward through the same forward raises
    y = m.forward_shared(v.to(DEV), q.to(DEV), ql.to(DEV), IMAGE_INDEX)
    torch.autograd.backward(y, torch.ones_like(y))
    with pytest.raises(RuntimeError, match="twice"):
        torch.autograd.backward(y, torch.ones_like(y))
    # a divisor of the caller's choice scales the loss
    with torch.no_grad():
        l2, _ = run_batch_shared(m, batch, 12, IMAGE_INDEX.tolist(), batch_divisor=14)
        l1, _ = run_batch_shared(m, batch, 12, IMAGE_INDEX.tolist())
    assert abs(float(l2) * 2 - float(l1)) < 1e-6
    with pytest.raises(IndexError):
        run_batch_shared(m, batch, 12, [0, 1, 2, 3, 0, 1, 1])


def test_existing_behaviour_untouched_and_unasked_images_get_zero_gradients():
    from dl_vqa_amd.train import soft_ce_loss_and_score
    g = Golden("tiny_plus")
    cfg = tiny_cfg(g.meta)
    v, q, ql = g.t["v"].to(DEV), g.t["q"].to(DEV), g.t["q_len"].to(DEV)
    a_idx, a_val = g.t["a_idx"].to(DEV), g.t["a_val"].to(DEV)

    def step(m):
        for p in m.parameters():
            p.grad = None
        y = m(v, q, ql)
        soft_ce_loss_and_score(y, a_idx, a_val)[0].backward()
        torch.cuda.synchronize()
        return y.detach().clone(), {k: p.grad.clone() for k, p in m.named_parameters()}

    y_f, g_f = step(build(cfg, g.meta["V"], g.sd).eval())
    m = build(cfg, g.meta["V"], g.sd).eval()
    vs, qs, qls, ais, avs = _fixture_batch(g)
    shared_step(m, vs, qs, qls, ais, avs, IMAGE_INDEX)
    assert len(m._pending) == 0
    y_m, g_m = step(m)                                                # a plain forward + backward afterwards: a fresh model's bits
    assert torch.equal(y_m, y_f)
    for k in g_f:
        assert torch.equal(g_m[k], g_f[k]), k
    # the inference calls still refuse training mode
    feats = m.encode_images(v)
    m.train()
    with pytest.raises(RuntimeError, match="training mode"):
        m.encode_images(v)
    with pytest.raises(RuntimeError, match="training mode"):
        m.answer(feats, q, ql, [0] * q.shape[0])
    m.eval()
    # an image nobody asks about: an all-zero image gradient, and nothing in the parameter gradients -- the same batch
    # without that image gives the same results (sums of the same terms plus exact zeros, in another order at most: the
    # parity tolerances of test_model_gpu apply)
    idx2 = torch.tensor([0, 1, 1, 0, 1])
    sel = torch.tensor([0, 1, 2, 1, 0])
    b5 = (g.t["q"][sel], g.t["q_len"][sel], g.t["a_idx"][sel], g.t["a_val"][sel])
    y3, l3, g3, dv3 = shared_step(m, g.t["v"][:3], *b5, idx2)
    y2, l2, g2, dv2 = shared_step(m, g.t["v"][:2], *b5, idx2)
    assert float(dv3[2].abs().max()) == 0.0 and float(dv3[:2].abs().max()) > 0
    assert float((y3 - y2).abs().max()) < 1e-5 and rel(dv3[:2], dv2) <= 2e-4
    for k in g3:
        assert grad_err(k, g3[k], g2[k]) < 2e-4, k
