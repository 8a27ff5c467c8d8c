"""GPU: training on cached image features -- vqa_gather_rows_drop against indexing the dropped bank (exact),
vqa_att_apply_gather_dscore against vqa_att_apply_gather_bwd (same bits), and VqaNet.forward_features /
train.run_batch_features against the CPU oracle run on the GATHERED images v[image_index].  In train mode the oracle gets the
masks the HIP path applies, extracted as data (tests/hip_masks.py): question-side sites one row per question, attention.drop
on v one row per row of the BANK gathered by image_index, and no image mask (the frozen encoder runs in eval mode).  The
fixture batches (BANK_INDEX) leave bank row 0 unasked, so in the train-mode test rows 1 and 2 sit in slots 0 and 1 and a
mask indexed by the slot in the batch instead of the bank row fails there."""
import pytest
import torch

from dl_vqa_amd import ImageFeatures, group_by_image
from tests.golden_util import TINY_CASES, Golden, tiny_cfg
from tests.test_model_gpu import ZERO_GRAD, build, grad_err
from tests.test_shared_train_gpu import QSEL, _full224_case, oracle_shared

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 0x5EED0FBA2C0FFEE

# 7 questions about rows 1 and 2 of a 3-row bank: a strict subset without row 0, with repeats
BANK_INDEX = torch.tensor([2, 1, 1, 2, 2, 1, 1])


def _ops():
    from dl_vqa_amd import ops
    return ops


# ----------------------------------------------------------------------------- vqa_gather_rows_drop
def _gather_case(n, M, row_len, p, rows=None, dst_off=0):
    """dst == src[rows] * mask[rows] with mask = vqa_dropout on ones of the whole bank: both sides are ONE fp32 multiply of
    the same element by 0 or 1/(1-p), so equality is exact."""
    ops = _ops()
    g = torch.Generator().manual_seed(n * 31 + M * 7 + row_len)
    src = torch.randn(M, row_len, generator=g).to(DEV)
    rows = torch.randint(0, M, (n,), generator=g) if rows is None else torch.as_tensor(rows)
    rows_d = rows.to(torch.int32).to(DEV)
    mask = ops.dropout(torch.ones(M, row_len, device=DEV), p, SEED)
    if p > 0:
        assert set(round(float(x), 4) for x in mask.unique().cpu()) == {0.0, round(1 / (1 - p), 4)}
    else:
        assert bool((mask == 1).all())
    buf = torch.full((n * row_len + 8,), 7.0, device=DEV)
    dst = buf[dst_off:dst_off + n * row_len].view(n, row_len)
    out = ops.gather_rows_drop(src, rows_d, p, SEED, out=dst)
    torch.cuda.synchronize()
    assert out.data_ptr() == dst.data_ptr()
    inside = (rows >= 0) & (rows < M)
    want = torch.zeros(n, row_len, device=DEV)
    sel = rows[inside].to(DEV)
    want[inside.to(DEV)] = src[sel] * mask[sel]
    assert torch.equal(dst, want)
    assert bool((buf[:dst_off] == 7).all()) and bool((buf[dst_off + n * row_len:] == 7).all())      # nothing outside dst
    again = ops.gather_rows_drop(src, rows_d, p, SEED)                                               # the same bits twice
    torch.cuda.synchronize()
    assert torch.equal(again, dst)
    return dst, src, mask


@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("n,M,row_len", [(3, 5, 224), (4, 6, 111), (2, 3, 173056), (1, 1, 8),
                                         (2 * 1024 * 1024 + 1000, 5, 4),        # float4 path: more rows than grid threads
                                         (64, 70, 173056),                      # bank-sized rows, the grid wraps inside rows
                                         (20000, 50, 111)])                     # scalar path, the grid wraps
def test_gather_rows_drop_is_exact(n, M, row_len, p):
    _gather_case(n, M, row_len, p)


@pytest.mark.parametrize("p", [0.0, 0.3])
def test_gather_rows_drop_repeats_bad_rows_and_misaligned_destinations(p):
    dst, src, mask = _gather_case(6, 4, 40, p, rows=[3, 3, 0, 3, 1, 0])                    # repeated rows
    assert torch.equal(dst[0], dst[1]) and torch.equal(dst[0], dst[3])
    dst, _, _ = _gather_case(5, 4, 40, p, rows=[1, 4, 0, -1, 3])                           # out of range: rows of zeros
    assert float(dst[1].abs().max()) == 0.0 and float(dst[3].abs().max()) == 0.0 and float(dst[0].abs().max()) > 0
    a, _, _ = _gather_case(5, 7, 64, p, rows=[6, 2, 2, 0, 5], dst_off=0)                   # 16-byte path
    b, _, _ = _gather_case(5, 7, 64, p, rows=[6, 2, 2, 0, 5], dst_off=1)                   # dst 4 bytes off: scalar path
    assert b.data_ptr() % 16 == 4 and torch.equal(a, b)
    if p > 0:                                                                              # the mask is per BANK row
        assert not torch.equal(mask[0], mask[1])


# ----------------------------------------------------------------------------- vqa_att_apply_gather_dscore
@pytest.mark.parametrize("N,B,P,C,G,asked", [(2, 7, 676, 256, 2, None), (3, 7, 70, 132, 3, None), (4, 11, 17, 64, 4, None),
                                             (50, 9, 70, 64, 2, (3, 17, 18, 40, 49))])
def test_apply_gather_dscore_has_the_bits_of_apply_gather_bwd(N, B, P, C, G, asked):
    ops = _ops()
    g = torch.Generator().manual_seed(B * 1000 + P + C)
    vn = torch.randn(N, P, C, generator=g).to(DEV)
    pr = torch.softmax(torch.randn(B, G, P, generator=g) * 2, dim=-1).to(DEV)
    ld = G * C + 12
    dout = torch.randn(B, ld, generator=g).to(DEV)
    if asked is None:
        img = torch.randint(0, N, (B,), generator=g)
    else:                                                           # a 50-row vn of which 5 rows are asked
        img = torch.tensor(asked)[torch.randint(0, len(asked), (B,), generator=g)]
        img[:len(asked)] = torch.tensor(asked)
    order, offsets = group_by_image(img, N)
    img_d = img.to(torch.int32).to(DEV)
    r_ref, r_new = torch.full((B, G), 7.0, device=DEV), torch.full((B, G), 9.0, device=DEV)
    ds_ref, _ = ops.att_apply_gather_bwd(dout, ld, pr, vn, img_d, order.to(DEV), offsets.to(DEV), rowsum=r_ref)
    ds_new = ops.att_apply_gather_dscore(dout, ld, pr, vn, img_d, rowsum=r_new)
    ds_nors = ops.att_apply_gather_dscore(dout, ld, pr, vn, img_d)
    torch.cuda.synchronize()
    assert float(ds_ref.abs().max()) > 0
    assert torch.equal(ds_new, ds_ref) and torch.equal(r_new, r_ref) and torch.equal(ds_nors, ds_ref)


# ----------------------------------------------------------------------------- the whole path
def _bank_batch(g):
    """The fixture's images as the bank; 7 questions about rows 1 and 2."""
    return g.t["v"], g.t["q"][QSEL], g.t["q_len"][QSEL], g.t["a_idx"][QSEL], g.t["a_val"][QSEL]


def _encode(m, v, **kw):
    was = m.training
    m.eval()
    feats = m.encode_images(v.to(DEV), **kw)
    m.train(was)
    return feats


def features_step(m, feats, q, ql, a_idx, a_val, image_index):
    from dl_vqa_amd.train import soft_ce_loss_and_score
    for p in m.parameters():
        p.grad = None
    y = m.forward_features(feats, q.to(DEV), ql.to(DEV), image_index)
    loss, _ = soft_ce_loss_and_score(y, a_idx.to(DEV), a_val.to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    return y.detach(), loss.detach(), {k: (None if p.grad is None else p.grad.clone()) for k, p in m.named_parameters()}


def _check_grads(tag, grads, g_ref, tol, do_option="+"):
    for k in grads:
        if k.startswith("image."):
            assert grads[k] is None, k                                  # not in the graph: torch leaves p.grad alone
            continue
        e = grad_err(k, grads[k], g_ref[k], do_option)
        print(f"[features] {tag} grad {k}: {e:.3e}")
        assert e < tol, (k, e)


@pytest.mark.parametrize("name", TINY_CASES)
def test_forward_features_matches_oracle_on_fixtures(name):
    """Eval mode, the fixture's images as the bank, 7 questions about rows 1 and 2: logits, loss and every non-image
    parameter gradient against the oracle on v[image_index], with the tolerances of
    test_forward_shared_matches_oracle_on_fixtures (logits 1e-5, loss 1e-5, gradients 2e-4)."""
    g = Golden(name)
    cfg = tiny_cfg(g.meta)
    m = build(cfg, g.meta["V"], g.sd).eval()
    v, q, ql, a_idx, a_val = _bank_batch(g)
    assert v.shape[0] >= 3 and 0 not in BANK_INDEX.tolist()
    y_ref, loss_ref, g_ref, _ = oracle_shared(g.sd, cfg, v, q, ql, a_idx, a_val, BANK_INDEX)
    feats = _encode(m, v)
    for k in m._image_names:                                            # a sentinel in the image slots of the flat buffer
        o, n = m._offsets[k]
        m._flat_grad[o:o + n].fill_(-7.5)
    flat_before = m._flat_grad.clone()
    y, loss, grads = features_step(m, feats, q, ql, a_idx, a_val, BANK_INDEX)
    err = float((y.cpu() - y_ref).abs().max())
    print(f"[features] {name}: logits max abs err {err:.3e}; loss {float(loss):.6f} vs {float(loss_ref):.6f}")
    assert y.shape == (7, cfg["max_answers"]) and err < 1e-5
    assert abs(float(loss) - float(loss_ref)) < 1e-5
    _check_grads(name, grads, g_ref, 2e-4, g.meta["do_option"])
    assert m._last_backward_direct is True and len(m._pending) == 0
    for k in grads:                                                     # the image slots of the flat buffer: not written
        if k.startswith("image."):
            o, n = m._offsets[k]
            assert torch.equal(m._flat_grad[o:o + n], flat_before[o:o + n]) and bool((flat_before[o:o + n] == -7.5).all()), k
    # the inference call on the same features
    y_ans = m.answer(feats, q.to(DEV), ql.to(DEV), BANK_INDEX)
    print(f"[features] {name}: logits bit-equal to answer(): {torch.equal(y_ans, y)}")
    assert float((y_ans - y).abs().max()) < 1e-5
    # outside a grad context: the same logits, nothing kept
    m._last_ctx = None
    with torch.no_grad():
        y_ng = m.forward_features(feats, q.to(DEV), ql.to(DEV), BANK_INDEX.tolist())
    assert torch.equal(y_ng, y) and m._last_ctx is None and len(m._pending) == 0
    with pytest.raises(IndexError):
        m.forward_features(feats, q.to(DEV), ql.to(DEV), [2, 1, 1, 2, 2, 1, v.shape[0]])
    with pytest.raises(ValueError, match="image_index entries"):
        m.forward_features(feats, q.to(DEV), ql.to(DEV), [1, 2])
    other = build(cfg, g.meta["V"], g.sd).eval()
    with pytest.raises(RuntimeError, match="belong elsewhere"):
        other.forward_features(feats, q.to(DEV), ql.to(DEV), BANK_INDEX)


def feature_masks(m, ctx, feats, image_index, T):
    """Question-side sites: one row per question.  attention.drop on v: the per-row masks of the BANK, gathered by
    image_index.  No image mask: image.drop is not applied to cached features."""
    from tests.hip_masks import hip_masks
    gs = feats.grid[0]
    masks = hip_masks(m._engine, ctx.seed, ctx.B, T, gs, DEV)
    masks["att_v"] = hip_masks(m._engine, ctx.seed, feats.N, T, gs, DEV)["att_v"][image_index]
    del masks["image"]
    return masks


@pytest.mark.parametrize("do_option", ["+", "*", "|"])
def test_forward_features_train_mode_matches_oracle_with_bank_row_masks(do_option):
    """Train mode, every site at p = 0.3, weights of the fixture; the masks the HIP path applies go to the oracle as data.
    Row 0 of the bank is unasked, so rows 1 and 2 sit in slots 0 and 1: an att_v mask indexed by the slot fails here.
    Tolerances of the shared train-mode test: logits 2e-5, loss 1e-5, gradients 2e-4."""
    from oracle import vqa_oracle as O
    g = Golden({"+": "tiny_plus", "*": "tiny_mul", "|": "tiny_cat"}[do_option])
    cfg = tiny_cfg(g.meta)
    m = build(cfg, g.meta["V"], g.sd).train()
    v, q, ql, a_idx, a_val = _bank_batch(g)
    feats = _encode(m, v, with_vprime=False)
    assert feats.vprime is None and m.training
    torch.manual_seed(123)
    rng = torch.get_rng_state()
    y, loss, grads = features_step(m, feats, q, ql, a_idx, a_val, BANK_INDEX)
    ctx = m._last_ctx
    assert ctx.p_att == 0.3 and ctx.seed != 0 and (ctx.N, ctx.B) == (2, 7)          # 2 distinct rows of the 3-row bank
    torch.set_rng_state(rng)
    assert ctx.seed == m._next_seed()                                 # one draw per training forward
    masks = feature_masks(m, ctx, feats, BANK_INDEX, q.shape[1])
    assert "image" not in masks
    for k, mk in masks.items():
        vals = set(round(float(x), 4) for x in mk.unique())
        assert vals == {0.0, round(1 / 0.7, 4)}, (k, vals)
        assert mk.shape[0] == 7, k
    y_ref, loss_ref, g_ref, _ = oracle_shared(g.sd, cfg, v, q, ql, a_idx, a_val, BANK_INDEX, masks=masks)
    err = float((y.cpu() - y_ref).abs().max())
    print(f"[features] train-mode ({do_option}) logits max abs err {err:.3e}; loss {float(loss):.6f} vs {float(loss_ref):.6f}")
    assert err < 2e-5
    assert abs(float(loss) - float(loss_ref)) < 1e-5
    assert float((y_ref - O.vqa_forward(g.sd, cfg, v[BANK_INDEX], q, ql)).abs().max()) > 1e-2     # the masks matter
    _check_grads(f"train-mode ({do_option})", grads, g_ref, 2e-4)
    # eval mode draws nothing
    m.eval()
    rng = torch.get_rng_state()
    with torch.no_grad():
        m.forward_features(feats, q.to(DEV), ql.to(DEV), BANK_INDEX)
    assert torch.equal(torch.get_rng_state(), rng)


@pytest.mark.parametrize("compute_dtype", ["fp32", "fp32x3"])
def test_forward_features_full224_matches_oracle(compute_dtype):
    """North-star architecture at 224 x 224, a bank of 2 images, 4 questions (image_index [1, 0, 0, 1]), train mode, against
    the float64 oracle with the HIP masks as data; tolerances of test_forward_shared_full224_matches_oracle: logits 1e-3,
    loss 1e-4, every gradient element 1e-3 of the largest."""
    from oracle import vqa_oracle as O
    meta, cfg, batch, _ = _full224_case()
    v, q, ql, a_idx, a_val = batch
    image_index = torch.tensor([1, 0, 0, 1])
    torch.manual_seed(meta["seed"])
    m = build(cfg, meta["V"], compute_dtype=compute_dtype).train()
    sd64 = {k: t.detach().cpu().double() for k, t in m.state_dict().items()}
    feats = _encode(m, v, with_vprime=False)
    y, loss, grads = features_step(m, feats, q, ql, a_idx, a_val, image_index)
    masks = feature_masks(m, m._last_ctx, feats, image_index, q.shape[1])
    y_ref, loss_ref, g_ref = O.loss_and_grads(sd64, cfg, v.double()[image_index], q, ql, a_idx, a_val, masks=masks)
    err = float((y.cpu().double() - y_ref).abs().max())
    print(f"[features] full224 train ({compute_dtype}) logits max abs err {err:.3e}; loss {float(loss):.6f} vs "
          f"{float(loss_ref):.6f}")
    assert err < 1e-3
    assert abs(float(loss) - float(loss_ref)) < 1e-4
    _check_grads(f"full224 train ({compute_dtype})", grads, g_ref, 1e-3)


def test_fused_adam_step_after_run_batch_features_matches_oracle():
    from oracle import vqa_oracle as O
    from dl_vqa_amd.train import FusedAdam, run_batch_features
    g = Golden("tiny_plus")
    cfg = tiny_cfg(g.meta)
    m = build(cfg, g.meta["V"], g.sd).eval()
    v, q, ql, a_idx, a_val = _bank_batch(g)
    _, loss_ref, g_ref = O.loss_and_grads(g.sd, cfg, v[BANK_INDEX], q, ql, a_idx, a_val)
    feats = _encode(m, v, with_vprime=False)
    batch = (None, q, a_idx, a_val, g.t["a_len"][QSEL], torch.arange(7), ql)          # the v entry is ignored
    opt = FusedAdam(m, lr=5e-4)
    loss, score = run_batch_features(m, batch, 12, feats, BANK_INDEX)
    opt.zero_grad()
    loss.backward()
    assert abs(float(loss.detach()) - float(loss_ref)) < 1e-5                  # divided by the 7 questions, as the oracle divides
    assert m._last_backward_direct is True
    for k, p in m.named_parameters():
        if k.startswith("image."):
            assert p.grad is None, k
            continue
        o, n = m._offsets[k]                                          # p.grad are views of the flat buffer
        assert p.grad.data_ptr() == m._flat_grad.data_ptr() + 4 * o, k
    opt.step()
    torch.cuda.synchronize()
    for k, p in m.named_parameters():
        o, n = m._offsets[k]
        if k.startswith("image."):                                    # frozen: value and moments untouched
            assert torch.equal(p.detach().cpu(), g.sd[k]), k
            assert float(opt.exp_avg[o:o + n].abs().max()) == 0.0 and float(opt.exp_avg_sq[o:o + n].abs().max()) == 0.0, k
            continue
        if k == ZERO_GRAD:
            continue
        ref = g.sd[k].clone()
        O.adam_step(ref, g_ref[k], torch.zeros_like(ref), torch.zeros_like(ref), 1, 5e-4)
        upd, upd_ref = p.detach().cpu() - g.sd[k], ref - g.sd[k]
        big = g_ref[k].abs() > 1e-3 * g_ref[k].abs().max()
        if bool(big.any()):
            assert float((upd - upd_ref)[big].abs().max()) < 1e-2 * 5e-4, k
    # the bank stays valid for this call after the in-place step: v' is recomputed from the stepped v_conv
    sd1 = {k: t.detach().cpu() for k, t in m.state_dict().items()}
    with torch.no_grad():
        y1 = m.forward_features(feats, q.to(DEV), ql.to(DEV), BANK_INDEX)
    assert float((y1.cpu() - O.vqa_forward(sd1, cfg, v[BANK_INDEX], q, ql)).abs().max()) < 1e-5
    # a second backward through the same forward raises
    y = m.forward_features(feats, q.to(DEV), ql.to(DEV), BANK_INDEX)
    torch.autograd.backward(y, torch.ones_like(y))
    with pytest.raises(RuntimeError, match="twice"):
        torch.autograd.backward(y, torch.ones_like(y))
    # a divisor of the caller's choice scales the loss
    with torch.no_grad():
        l2, _ = run_batch_features(m, batch, 12, feats, BANK_INDEX.tolist(), batch_divisor=14)
        l1, _ = run_batch_features(m, batch, 12, feats, BANK_INDEX.tolist())
    assert abs(float(l2) * 2 - float(l1)) < 1e-6
    with pytest.raises(IndexError):
        run_batch_features(m, batch, 12, feats, [0, 1, 2, 3, 0, 1, 1])


def test_forward_features_does_not_depend_on_the_rest_of_the_bank():
    """The same batch against a bank that holds only the asked images and against one with other rows interleaved: logits
    within 1e-5, gradients within 2e-4 (eval mode: the att_v masks of the two banks differ by construction)."""
    g = Golden("tiny_plus")
    cfg = tiny_cfg(g.meta)
    m = build(cfg, g.meta["V"], g.sd).eval()
    v, q, ql, a_idx, a_val = _bank_batch(g)
    small = _encode(m, v[[1, 2]], with_vprime=False)                                  # rows: image 1, image 2
    big = _encode(m, v[[0, 1, 0, 0, 2, 1, 0]], with_vprime=False)                     # image 1 at row 1, image 2 at row 4
    to_small = torch.tensor([0, 0, 1])[BANK_INDEX]
    to_big = torch.tensor([0, 1, 4])[BANK_INDEX]
    y_s, l_s, g_s = features_step(m, small, q, ql, a_idx, a_val, to_small)
    y_b, l_b, g_b = features_step(m, big, q, ql, a_idx, a_val, to_big)
    assert float((y_s - y_b).abs().max()) < 1e-5 and abs(float(l_s) - float(l_b)) < 1e-5
    for k in g_s:
        if k.startswith("image."):
            assert g_s[k] is None and g_b[k] is None
        else:
            assert grad_err(k, g_b[k], g_s[k]) < 2e-4, k


def test_features_step_leaves_everything_else_as_it_was():
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
    vb, qs, qls, ais, avs = _bank_batch(g)
    feats = m.encode_images(v)
    features_step(m, feats, qs, qls, ais, avs, BANK_INDEX)
    assert len(m._pending) == 0
    y_m, g_m = step(m)                                                # a plain forward + backward afterwards: a fresh model's bits
    assert torch.equal(y_m, y_f)
    for k in g_f:
        assert torch.equal(g_m[k], g_f[k]), k
    # a bank encoded in chunks is the bank encoded at once, bit for bit
    parts = [m.encode_images(v[:1]), m.encode_images(v[1:])]
    joined = ImageFeatures.cat(parts)
    assert joined.N == feats.N and joined.grid == feats.grid
    assert torch.equal(joined.vn, feats.vn) and torch.equal(joined.vprime, feats.vprime)
    each = [b % feats.N for b in range(q.shape[0])]
    assert torch.equal(m.answer(joined, q, ql, each), m.answer(feats, q, ql, each))
    # without v': the same vn bits, a bank forward_features serves and answer() refuses
    bank = m.encode_images(v, with_vprime=False)
    assert bank.vprime is None and torch.equal(bank.vn, feats.vn)
    assert ImageFeatures.cat([parts[0], m.encode_images(v[1:], with_vprime=False)]).vprime is None
    with pytest.raises(RuntimeError, match="with_vprime"):
        m.answer(bank, q, ql, [0] * q.shape[0])
    with pytest.raises(RuntimeError, match="with_vprime"):
        m.predict(bank, q, ql, [0] * q.shape[0])
    with pytest.raises(RuntimeError, match="with_vprime"):
        m.answer_pairs(bank, m.encode_questions(q, ql), [0], [0])
    with torch.no_grad():
        assert torch.equal(m.forward_features(bank, qs.to(DEV), qls.to(DEV), BANK_INDEX),
                           m.forward_features(feats, qs.to(DEV), qls.to(DEV), BANK_INDEX))
