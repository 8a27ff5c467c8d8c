"""GPU: many questions per image -- vqa_att_score_grouped_fwd and vqa_att_apply_gather_fwd against float64, and
VqaNet.encode_images / answer against the reference's stored logits and the CPU oracle run on v[image_index] (the new
path is never judged by the HIP forward alone; that comparison is an additional check where it appears)."""
import pytest
import torch

from dl_vqa_amd import group_by_image
from tests.golden_util import TINY_CASES, Golden, full_cfg, full_inputs, tiny_cfg
from tests.test_kernels_gpu import check

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _ops():
    from dl_vqa_amd import ops
    return ops


def rel(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-30)


def build(cfg, V, sd=None, compute_dtype="fp32"):
    from dl_vqa_amd import VqaNet
    m = VqaNet(cfg, V, compute_dtype=compute_dtype)
    if sd is not None:
        m.load_state_dict(sd)
    return m.to(DEV)


def _grouping(kind, N, B, g):
    if kind == "empty":          # image N-1 (and, for N > 2, image 1) has no question; every other one has some
        pool = [n for n in range(N) if n != N - 1 and (N <= 2 or n != 1)]
        return torch.tensor(pool)[torch.randint(0, len(pool), (B,), generator=g)]
    if kind == "single":         # one image holds every question
        return torch.full((B,), N // 2, dtype=torch.int64)
    return torch.randint(0, N, (B,), generator=g)      # shuffled


def score_reference(vp, qp, wx, bx, img, P, mode):
    """float64 evaluation of the formulas in include/vqa_hip.h: [B, G, P]."""
    N = vp.shape[0] // P
    mid = vp.shape[1]
    v = vp.double().view(N, P, mid)[img]                        # [B, P, mid]
    q = qp.double()[:, None, :]                                 # [B, 1, mid]
    w, b = wx.double(), bx.double()
    if mode == 0:
        s = torch.relu(v + q) @ w.t()
    elif mode == 1:
        s = torch.relu(v * q) @ w.t()
    else:
        s = torch.relu(v) @ w[:, :mid].t() + torch.relu(q) @ w[:, mid:].t()
    return (s + b).permute(0, 2, 1)


# ----------------------------------------------------------------------------- item 5: the grouped score kernel
@pytest.mark.parametrize("kind", ["empty", "single", "shuffled"])
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("N,B,P,mid,G", [(3, 7, 4, 24, 2), (2, 9, 676, 1024, 2), (5, 5, 169, 256, 1),
                                         (4, 33, 2916, 1024, 2), (3, 6, 100, 520, 4), (2, 5, 37, 2048, 3)])
def test_grouped_score_matches_float64(N, B, P, mid, G, mode, kind):
    ops = _ops()
    g = torch.Generator().manual_seed(N * 1000 + B * 10 + mode)
    vp = torch.randn(N * P, mid, generator=g)
    qp = torch.randn(B, mid, generator=g)
    wx = torch.randn(G, 2 * mid if mode == 2 else mid, generator=g)
    bx = torch.randn(G, generator=g)
    img = _grouping(kind, N, B, g)
    order, offsets = group_by_image(img, N)
    want = score_reference(vp, qp, wx, bx, img, P, mode)
    score = ops.att_score_grouped_fwd(vp.to(DEV), qp.to(DEV), wx.to(DEV), bx.to(DEV), order.to(DEV), offsets.to(DEV),
                                      N, B, P, mode)
    torch.cuda.synchronize()
    assert score.shape == (B, G, P)
    check(f"att_score_grouped {N,B,P,mid,G} mode {mode} {kind}", score, want, 3e-6)      # every element


# ----------------------------------------------------------------------------- item 6: apply with an image index
@pytest.mark.parametrize("B,P,C,G", [(2, 676, 256, 2), (2, 70, 130, 3), (3, 100, 72, 1), (2, 17, 64, 4), (1, 65, 8, 2)])
def test_apply_gather_matches_float64_and_the_plain_kernel(B, P, C, G):
    ops = _ops()
    g = torch.Generator().manual_seed(B * 1000 + P + C)
    N, Bq = B, 2 * B + 3                                        # more questions than images, random image per question
    vn = torch.randn(N, P, C, generator=g)
    score = torch.randn(Bq, G, P, generator=g) * 2
    img = torch.randint(0, N, (Bq,), generator=g)
    pr = torch.softmax(score.double(), dim=-1)
    ref = torch.einsum("bgp,bpc->bgc", pr, vn.double()[img]).reshape(Bq, G * C)
    ld = G * C + 12
    out = torch.full((Bq, ld), 7.0, device=DEV)
    probs = ops.att_apply_gather_fwd(score.to(DEV), vn.to(DEV), img.to(torch.int32).to(DEV), out, ld)
    torch.cuda.synchronize()
    check(f"att_apply_gather probs {B,P,C,G}", probs, pr, 3e-6)
    check(f"att_apply_gather out {B,P,C,G}", out[:, :G * C], ref, 3e-6)
    assert bool((out[:, G * C:] == 7.0).all())
    # img = arange(B): the plain kernel's results, bit for bit
    s2 = score[:B].contiguous().to(DEV)
    out_g = torch.full((B, ld), 7.0, device=DEV)
    out_p = torch.full((B, ld), 7.0, device=DEV)
    probs_g = ops.att_apply_gather_fwd(s2, vn.to(DEV), torch.arange(B, dtype=torch.int32, device=DEV), out_g, ld)
    probs_p = ops.att_apply_fwd(s2, vn.to(DEV), out_p, ld)
    torch.cuda.synchronize()
    assert torch.equal(probs_g, probs_p) and torch.equal(out_g, out_p)


# ----------------------------------------------------------------------------- item 7: the whole path on the fixtures
@pytest.mark.parametrize("name", TINY_CASES)
def test_answer_matches_reference_and_oracle_on_fixtures(name):
    from oracle import vqa_oracle as O
    g = Golden(name)
    cfg = tiny_cfg(g.meta)
    m = build(cfg, g.meta["V"], g.sd).eval()
    v, q, ql = g.t["v"], g.t["q"], g.t["q_len"]
    assert v.shape[0] >= 3
    image_index = torch.tensor([0, 1, 2, 2, 0, 1, 1])
    qsel = torch.tensor([0, 1, 2, 0, 1, 2, 1])
    qq, qql = q[qsel], ql[qsel]
    feats = m.encode_images(v[:3].to(DEV))
    logits, att = m.answer(feats, qq.to(DEV), qql.to(DEV), image_index, return_attention=True)
    torch.cuda.synchronize()
    assert not logits.requires_grad and not att.requires_grad and not feats.vn.requires_grad
    gh, gw = feats.grid
    assert logits.shape == (7, cfg["max_answers"]) and att.shape == (7, 2, gh, gw) and feats.N == 3
    # rows 0-2: the fixture's own (image, question) pairs -> the reference's stored logits
    e_ref = float((logits[:3].cpu() - g.t["logits"][:3]).abs().max())
    stages = {}
    y_or = O.vqa_forward(g.sd, cfg, v[image_index], qq, qql, stages=stages)
    e_or = float((logits.cpu() - y_or).abs().max())
    e_att = rel(att.reshape(7, 2, -1), stages["probs"])
    print(f"[multi-q] {name}: logits vs reference {e_ref:.3e}, vs oracle {e_or:.3e}, attention rel {e_att:.3e}")
    assert e_ref < 1e-5
    assert e_or < 1e-5
    assert e_att < 2e-5
    assert float((att.sum(dim=(2, 3)) - 1).abs().max()) < 1e-5
    # additional: the one-image-per-question forward on the gathered images
    with torch.no_grad():
        y_fwd = m(v[image_index].to(DEV), qq.to(DEV), qql.to(DEV))
    assert float((logits - y_fwd).abs().max()) < 1e-5


# ----------------------------------------------------------------------------- item 8: north-star architecture
def _full224(compute_dtype):
    g = Golden("full224_seed1")
    meta = g.meta
    torch.manual_seed(meta["seed"])
    m = build(full_cfg(meta["A"]), meta["V"], compute_dtype=compute_dtype).eval()
    v, q, ql, _, _, _ = full_inputs(meta)
    return g, m, v, q, ql


@pytest.mark.parametrize("compute_dtype", ["fp32", "fp32x3"])
def test_answer_full224_reference_and_oracle(compute_dtype):
    from oracle import vqa_oracle as O
    g, m, v, q, ql = _full224(compute_dtype)
    image_index = torch.tensor([0, 1, 1, 0])
    qsel = torch.tensor([0, 1, 0, 1])
    qq, qql = q[qsel], ql[qsel]
    feats = m.encode_images(v.to(DEV))
    logits = m.answer(feats, qq.to(DEV), qql.to(DEV), image_index)
    # the score stage, through the schedule the public call runs
    order, offsets = group_by_image(image_index, 2)
    _, probs, score = m._engine.answer(m._param_dict(), feats, qq.to(DEV), qql.to(DEV), order.to(DEV), offsets.to(DEV),
                                       image_index.to(torch.int32).to(DEV))
    torch.cuda.synchronize()
    e_ref = float((logits[:2].cpu() - g.t["logits"]).abs().max())
    e_sc = rel(score[:2].reshape(2, 2, -1), g.t["attention"].reshape(2, 2, -1))
    sd = {k: t.detach().cpu() for k, t in m.state_dict().items()}
    y_or = O.vqa_forward(sd, full_cfg(g.meta["A"]), v[image_index], qq, qql)
    e_or = float((logits.cpu() - y_or).abs().max())
    print(f"[multi-q] full224 ({compute_dtype}): logits vs reference {e_ref:.3e}, score rel {e_sc:.3e}, vs oracle {e_or:.3e}")
    assert e_ref < 1e-3
    assert e_sc < 1e-4
    assert e_or < 1e-3
    assert m._last_ctx is None


# ----------------------------------------------------------------------------- item 9: order invariance, bit for bit
def _assert_order_invariant(m, feats, q, ql, image_index, seed):
    B = q.shape[0]
    y0, a0 = m.answer(feats, q.to(DEV), ql.to(DEV), image_index, return_attention=True)
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(seed))
    y1, a1 = m.answer(feats, q[perm].to(DEV), ql[perm].to(DEV), image_index[perm], return_attention=True)
    torch.cuda.synchronize()
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(B)
    assert torch.equal(y1[inv.to(DEV)], y0)
    assert torch.equal(a1[inv.to(DEV)], a0)


def test_order_invariance_full224():
    _, m, v, q, ql = _full224("fp32")
    feats = m.encode_images(v.to(DEV))
    _assert_order_invariant(m, feats, q[[0, 1, 0, 1]], ql[[0, 1, 0, 1]], torch.tensor([0, 1, 1, 0]), seed=3)


def test_order_invariance_16_images_128_questions():
    from oracle import vqa_oracle as O
    V, N, B, T = 500, 16, 128, 14
    torch.manual_seed(9)
    m = build(full_cfg(100), V).eval()
    v, q, _, _, _, _, ql = O.synthetic_batch(B, 64, T, V, 100, seed=11)
    feats = m.encode_images(v[:N].to(DEV))
    image_index = torch.randint(0, N, (B,), generator=torch.Generator().manual_seed(12))
    _assert_order_invariant(m, feats, q, ql, image_index, seed=13)
    # CUDA image_index (one synchronising copy) and a plain list give the same rows
    y_a = m.answer(feats, q.to(DEV), ql.to(DEV), image_index.to(DEV))
    y_b = m.answer(feats, q.to(DEV), ql.to(DEV), image_index.tolist())
    assert torch.equal(y_a, y_b)


# ----------------------------------------------------------------------------- item 10: existing behaviour untouched
def test_forward_backward_unchanged_after_the_new_calls():
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
    y_f, g_f = step(fresh)

    m = build(cfg, g.meta["V"], g.sd).eval()
    m._ensure_flat()
    flat_grad = m._flat_grad
    flat_grad.fill_(3.0)
    torch.manual_seed(77)
    rng = torch.get_rng_state()
    feats = m.encode_images(v)
    y_a = m.answer(feats, q, ql, [(b + 1) % feats.N for b in range(q.shape[0])])
    torch.cuda.synchronize()
    assert m._last_ctx is None and len(m._pending) == 0
    assert m._flat_grad is flat_grad and bool((flat_grad == 3.0).all())
    assert torch.equal(torch.get_rng_state(), rng)                  # the dropout seed stream was not drawn from
    assert all(p.grad is None for p in m.parameters())
    assert y_a.shape == y_f.shape
    flat_grad.zero_()
    y_m, g_m = step(m)
    assert torch.equal(y_m, y_f)
    for k in g_f:
        assert torch.equal(g_m[k], g_f[k]), k

    # features of another model instance are refused; so are features of a model that was re-flattened since
    with pytest.raises(RuntimeError, match="belong elsewhere"):
        fresh.answer(feats, q, ql, [0] * q.shape[0])
    m._flatten(torch.device(DEV))
    with pytest.raises(RuntimeError, match="belong elsewhere"):
        m.answer(feats, q, ql, [0] * q.shape[0])
    # errors raised before any launch
    feats = m.encode_images(v)
    with pytest.raises(IndexError):
        m.answer(feats, q, ql, [0] * (q.shape[0] - 1) + [feats.N])
    with pytest.raises(IndexError):
        m.answer(feats, torch.full_like(q, g.meta["V"]).cpu(), ql, [0] * q.shape[0])
    with pytest.raises(RuntimeError, match="question length"):
        m.answer(feats, q, torch.zeros_like(ql).cpu(), [0] * q.shape[0])
    m.train()
    with pytest.raises(RuntimeError, match="training mode"):
        m.answer(feats, q, ql, [0] * q.shape[0])


# ----------------------------------------------------------------------------- item 11: fp16 images
def test_fp16_images_encode_bit_for_bit(monkeypatch):
    from dl_vqa_amd import ops
    from oracle import vqa_oracle as O
    torch.manual_seed(5)
    m = build(full_cfg(100), 60).eval()
    v, _, _, _, _, _, _ = O.synthetic_batch(2, 96, 6, 60, 100, seed=4)
    assert ops.conv0_supported(3, 96, 96, 64, 1)
    v16 = v.half()
    f32 = m.encode_images(v16.float().to(DEV))

    def boom(*a, **k):
        raise AssertionError("vqa_half_to_float must not run at conv0-supported shapes")
    monkeypatch.setattr(ops, "half_to_float", boom)
    f16 = m.encode_images(v16.to(DEV))
    torch.cuda.synchronize()
    assert torch.equal(f16.vn, f32.vn) and torch.equal(f16.vprime, f32.vprime) and f16.grid == f32.grid
