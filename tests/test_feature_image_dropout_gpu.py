"""GPU: image dropout when training on cached image features.

vqa_gather_rows_drop_norm / _f16 against the float64 formula of tests/feature_dropout_ref.py, with the masks the kernel applies
extracted as data (vqa_dropout on ones of the whole bank, as tests/hip_masks.py does), plus the properties that hold bit for
bit.  VqaNet.forward_features(..., image_dropout=True) against the CPU oracle on the gathered images with the image mask
INCLUDED -- the oracle drops the pooled features and normalises them, the HIP path drops and renormalises the cached,
normalised ones -- and against forward_shared under the same seed.  With the flag off, in eval mode or at image.dropout = 0
nothing moves: the same bits as before.

`python -m tests.test_feature_image_dropout_gpu` prints the observed kernel error (profiles/feature_image_dropout_parity.txt)."""
import functools

import pytest
import torch

from tests.feature_dropout_ref import drop_norm, kept_norms
from tests.golden_util import Golden, tiny_cfg
from tests.test_feature_train_gpu import BANK_INDEX, _bank_batch, _check_grads, _encode
from tests.test_model_gpu import build
from tests.test_shared_train_gpu import QSEL, _full224_case, oracle_shared, shared_step

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED_IMG, SEED_ATT = 0x5EED0FBA2C0FFEE, 0x0DDBA11C0FFEE123
ULP = 2.0 ** -24

# (n, M, P, C): the smallest case; 21 feature rows (the tail of the four-rows-in-flight group); 63 quads (one idle lane); the
# full register path; the first shape of the general path; a wide general-path row
SHAPES = [(1, 1, 1, 4), (3, 5, 7, 8), (2, 3, 5, 252), (2, 3, 3, 256), (2, 3, 3, 260), (1, 2, 2, 512)]


def _ops():
    from dl_vqa_amd import ops
    return ops


@functools.lru_cache(maxsize=None)
def _bank(M, P, C):
    """An fp32 bank built on the CPU from a fixed seed: L2-normalised rows, about half the entries zero, the others from
    [0.5, 1.5) before the normalisation -- so every non-zero entry is at least 0.5 / (1.5 * sqrt(512)) = 1.4e-2 and the kept
    part of a row is either all zero or far above 1e-3.  Shared by the tests: nobody writes to it."""
    g = torch.Generator().manual_seed(M * 100003 + P * 1009 + C)
    x = (0.5 + torch.rand(M, P, C, generator=g)) * (torch.rand(M, P, C, generator=g) < 0.5)
    return x / (x.norm(dim=-1, keepdim=True) + 1e-12)


def _rows(n, M):
    """(base [n]: the shape as the table states it, in-range and distinct where M allows; full [n + 2]: base, then a repeat of
    its first entry and one entry out of range)."""
    base = [(M - 1 - 2 * j) % M for j in range(n)]
    return base, base + [base[0], M if n % 2 else -1]


def _mask(M, P, C, p, seed):
    """The keep-scale mask of the whole bank, as data."""
    if p == 0:
        return torch.ones(M, P, C)
    m = _ops().dropout(torch.ones(M, P, C, device=DEV), p, seed).cpu()
    assert set(round(float(x), 4) for x in m.unique()) <= {0.0, round(1 / (1 - p), 4)}
    return m


def _run(bank, rows, p, p2, with_vdrop):
    rows_d = torch.tensor(rows, dtype=torch.int32, device=DEV)
    out = _ops().gather_rows_drop_norm(bank.to(DEV), rows_d, p, SEED_IMG, drop2=(p2, SEED_ATT) if with_vdrop else None)
    torch.cuda.synchronize()
    return tuple(t.cpu() for t in out) if with_vdrop else (out.cpu(), None)


def kernel_case(n, M, P, C, p, p2, half):
    """Every assertion of one kernel case; returns the observed max |err| / |ref| of vn_out in units of 2^-24."""
    bank32 = _bank(M, P, C)
    bank = bank32.half() if half else bank32
    values = bank.float()                                   # what the kernel computes on
    base, rows = _rows(n, M)
    mask_img, mask_att = _mask(M, P, C, p, SEED_IMG), _mask(M, P, C, p2, SEED_ATT)
    # on the CPU, before the kernel runs: every compared row's kept part is all zero or has norm >= 1e-3
    kept = kept_norms(values, rows, mask_img)
    assert bool(((kept == 0) | (kept >= 1e-3)).all()), float(kept[kept > 0].min())
    ref_vn, ref_vd = drop_norm(values, rows, mask_img, mask_att)

    vn, vd = _run(bank, rows, p, p2, True)
    vn_only, none = _run(bank, rows, p, p2, False)
    assert none is None and torch.equal(vn_only, vn)        # vdrop_out absent: the same vn_out
    assert vn.shape == (n + 2, P, C) and vn.dtype == torch.float32 and not bool(torch.isnan(vn).any())
    err = (vn.double() - ref_vn).abs()
    nz = ref_vn != 0
    worst = float((err[nz] / ref_vn.abs()[nz]).max()) / ULP if bool(nz.any()) else 0.0
    print(f"[image-drop] {(n, M, P, C)} p {p} p2 {p2} {'f16' if half else 'f32'}: vn_out max |err|/|ref| = {worst:.3f} x 2^-24")
    assert bool((err <= 16 * ULP * ref_vn.abs()).all()), worst
    # ---- exact properties
    inside = torch.tensor([0 <= r < M for r in rows])
    sel = torch.tensor([min(max(r, 0), M - 1) for r in rows])
    assert bool((vn[inside][mask_img[sel][inside] == 0] == 0).all())                         # zero where the image mask drops
    assert torch.equal(vd, vn * mask_att[sel])                                               # one fp32 multiply on both sides
    assert torch.equal(vn[n], vn[0]) and torch.equal(vd[n], vd[0])                           # the repeat
    assert float(vn[n + 1].abs().max()) == 0 and float(vd[n + 1].abs().max()) == 0           # out of range: zeros
    assert float(vn[0].abs().max()) > 0 or float(kept[0].max()) == 0
    # the shape as stated (n entries): a prefix of the same rows gives the same bits
    vn_b, vd_b = _run(bank, base, p, p2, True)
    assert torch.equal(vn_b, vn[:n]) and torch.equal(vd_b, vd[:n])
    # permuting rows permutes the output rows
    perm = list(reversed(range(n + 2)))
    vn_p, vd_p = _run(bank, [rows[i] for i in perm], p, p2, True)
    assert torch.equal(vn_p, vn[perm]) and torch.equal(vd_p, vd[perm])
    # a bank row zeroed wherever its mask keeps: zeros, no NaN; the other rows keep their bits
    dead = bank.clone()
    dead[rows[0]] = dead[rows[0]] * (mask_img[rows[0]] == 0).to(dead.dtype)
    vn_z, vd_z = _run(dead, rows, p, p2, True)
    hit = torch.tensor([r == rows[0] for r in rows])
    assert not bool(torch.isnan(vn_z).any()) and not bool(torch.isnan(vd_z).any())
    assert float(vn_z[hit].abs().max()) == 0 and float(vd_z[hit].abs().max()) == 0
    assert torch.equal(vn_z[~hit], vn[~hit]) and torch.equal(vd_z[~hit], vd[~hit])
    # overwriting the unasked bank rows changes no output bit
    unasked = [r for r in range(M) if r not in rows]
    if unasked:
        other = bank.clone()
        other[unasked] = float("nan")
        vn_o, vd_o = _run(other, rows, p, p2, True)
        assert torch.equal(vn_o, vn) and torch.equal(vd_o, vd)
    # the half bank gives the bits of the fp32 bank holding .float() of it
    if half:
        vn_w, vd_w = _run(values, rows, p, p2, True)
        assert torch.equal(vn_w, vn) and torch.equal(vd_w, vd)
    return worst


@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("p2", [0.0, 0.3])
@pytest.mark.parametrize("p", [0.3, 0.5])
@pytest.mark.parametrize("n,M,P,C", SHAPES)
def test_gather_rows_drop_norm_matches_float64_and_its_exact_properties(n, M, P, C, p, p2, half):
    """vn_out against drop_norm in float64: |err| <= 16 * 2^-24 * |ref| per element.  fp32 roundings on positive terms: one for
    the mask product; at most eleven across the sum of squares (squares, in-lane sum, six butterfly steps), halved by the
    square root; then square root, add, reciprocal and the final product: 1 + 5.5 + 4 < 16 half-ulps of 2^-24.  vdrop_out
    present and absent both run; the exact properties are compared with torch.equal."""
    kernel_case(n, M, P, C, p, p2, half)


def test_the_fixture_banks_have_zeros_and_are_normalised():
    for n, M, P, C in SHAPES:
        b = _bank(M, P, C)
        live = b.norm(dim=-1) > 0
        assert float((b[live].norm(dim=-1) - 1).abs().max()) < 1e-6
        if b.numel() >= 64:
            assert 0.3 < float((b == 0).float().mean()) < 0.7
        nz = b[b != 0]
        assert nz.numel() == 0 or float(nz.min()) >= 1e-2


# ----------------------------------------------------------------------------- the whole path
def step(m, feats, q, ql, a_idx, a_val, image_index, *flag, **kw):
    from dl_vqa_amd.train import soft_ce_loss_and_score
    for p in m.parameters():
        p.grad = None
    y = m.forward_features(feats, q.to(DEV), ql.to(DEV), image_index, *flag, **kw)
    loss, _ = soft_ce_loss_and_score(y, a_idx.to(DEV), a_val.to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    return y.detach(), loss.detach(), {k: (None if p.grad is None else p.grad.clone()) for k, p in m.named_parameters()}


def seed_masks(m, seed, B, feats, image_index, T):
    """Question-side sites: one row per question.  Image-side sites (image.drop and attention.drop on v): the per-row masks of
    the BANK, gathered by image_index."""
    from tests.hip_masks import hip_masks
    gs = feats.grid[0]
    masks = hip_masks(m._engine, seed, B, T, gs, DEV)
    per_row = hip_masks(m._engine, seed, feats.N, T, gs, DEV)
    for site in ("image", "att_v"):
        masks[site] = per_row[site][image_index]
    return masks


def bank_masks(m, ctx, feats, image_index, T):
    return seed_masks(m, ctx.seed, ctx.B, feats, image_index, T)


def _same(a, b):
    (ya, la, ga), (yb, lb, gb) = a, b
    assert torch.equal(ya, yb) and torch.equal(la, lb)
    for k in ga:
        assert (ga[k] is None and gb[k] is None) or torch.equal(ga[k], gb[k]), k


@pytest.mark.parametrize("do_option", ["+", "*", "|"])
def test_image_dropout_on_the_bank_matches_oracle_and_forward_shared(do_option):
    """Train mode, every site at p = 0.3, the fixture's images as the bank, row 0 unasked (rows 1 and 2 sit in slots 0 and 1).
    The masks go to the oracle as data and INCLUDE the image mask of the asked bank rows.  Tolerances of the existing
    train-mode test: logits 2e-5, loss 1e-5, non-image gradients 2e-4.  forward_shared on the images under the same seed: each
    within 2e-5 of the same oracle logits, so within 4e-5 of each other."""
    from oracle import vqa_oracle as O
    g = Golden({"+": "tiny_plus", "*": "tiny_mul", "|": "tiny_cat"}[do_option])
    cfg = tiny_cfg(g.meta)
    m = build(cfg, g.meta["V"], g.sd).train()
    v, q, ql, a_idx, a_val = _bank_batch(g)
    feats = _encode(m, v, with_vprime=False)
    for k in m._image_names:                                            # a sentinel in the image slots of the flat buffer
        o, n = m._offsets[k]
        m._flat_grad[o:o + n].fill_(-7.5)
    flat_before = m._flat_grad.clone()
    torch.manual_seed(123)
    rng = torch.get_rng_state()
    y, loss, grads = step(m, feats, q, ql, a_idx, a_val, BANK_INDEX, image_dropout=True)
    ctx = m._last_ctx
    assert ctx.p_att == 0.3 and ctx.seed != 0 and (ctx.N, ctx.B) == (2, 7)
    assert ctx.vn.shape[0] == 2 and ctx.vn.data_ptr() != feats.vn.data_ptr()          # the dropped rows, read at the slot
    assert ctx.img.tolist() == [1, 0, 0, 1, 1, 0, 0] and ctx.rows.tolist() == [1, 2]
    torch.set_rng_state(rng)
    assert ctx.seed == m._next_seed()                                   # one draw per training forward
    masks = bank_masks(m, ctx, feats, BANK_INDEX, q.shape[1])
    for k, mk in masks.items():
        assert set(round(float(x), 4) for x in mk.unique()) == {0.0, round(1 / 0.7, 4)}, k
        assert mk.shape[0] == 7, k
    y_ref, loss_ref, g_ref, _ = oracle_shared(g.sd, cfg, v, q, ql, a_idx, a_val, BANK_INDEX, masks=masks)
    without = {k: mk for k, mk in masks.items() if k != "image"}
    gap = float((y_ref - O.vqa_forward(g.sd, cfg, v[BANK_INDEX], q, ql, masks=without)).abs().max())
    err = float((y.cpu() - y_ref).abs().max())
    print(f"[image-drop] train-mode ({do_option}) logits max abs err {err:.3e}; loss {float(loss):.6f} vs {float(loss_ref):.6f}; "
          f"the image mask moves the oracle's logits by {gap:.3e}")
    assert gap > 1e-3                                                   # the image mask matters
    assert err < 2e-5
    assert abs(float(loss) - float(loss_ref)) < 1e-5
    _check_grads(f"image-drop ({do_option})", grads, g_ref, 2e-4)
    assert m._last_backward_direct is True and len(m._pending) == 0
    for k in m._image_names:                                            # the image slots of the flat buffer: not written
        o, n = m._offsets[k]
        assert torch.equal(m._flat_grad[o:o + n], flat_before[o:o + n]) and bool((flat_before[o:o + n] == -7.5).all()), k
    # the same step through forward_shared on the images, same seed
    torch.manual_seed(123)
    y_sh, _, _, _ = shared_step(m, v, q, ql, a_idx, a_val, BANK_INDEX, want_dv=False)
    assert m._last_ctx.seed == ctx.seed
    err_sh = float((y_sh.cpu() - y_ref).abs().max())
    both = float((y_sh - y).abs().max())
    print(f"[image-drop] train-mode ({do_option}) forward_shared vs oracle {err_sh:.3e}, vs forward_features {both:.3e}")
    assert err_sh < 2e-5 and both < 4e-5


# The torch seed under which the north-star case draws its dropout seed, and the margins asserted for it (see the test).
FULL224_TORCH_SEED, ATT_MARGIN, CLS_MARGIN = 1366, 3e-7, 1e-6


def test_image_dropout_full224_matches_oracle():
    """North-star architecture at 224 x 224, a bank of 2 images, 4 questions, fp32, train mode, image_dropout=True, against the
    float64 oracle with the HIP masks (the image mask included) as data; tolerances of
    test_forward_features_full224_matches_oracle: logits 1e-3, loss 1e-4, every gradient element 1e-3 of the largest.

    The dropout seed.  A parameter gradient is discontinuous where a ReLU pre-activation crosses zero, and the attention stage
    has 4 x 1024 x 676 = 2.8 million of them (v' + q', median magnitude 0.06): in every batch a few lie within 1e-7 of zero,
    which is the fp32 error of such a value -- v' is 256 multiply-adds on partial sums below 0.21, a random-walk bound of
    16 x 2^-24 x 0.21 = 2e-7, plus about 1e-7 from the error of its fp32 inputs; measured on an MI355X against the float64
    product of the same fp32 operands: at most 1.0e-7, median 3.3e-9.  One flipped element moves an entry of the v_conv and
    q_lin gradients by about dscore x wx x v = 1e-7 .. 1e-5, against a largest entry of 3e-6 (those gradients are sums over
    positions of terms that nearly cancel: tests/test_shared_train_gpu.py).  Under the seed of the existing test
    (torch.manual_seed(meta["seed"])) the ORACLE's nearest pre-activation is 8.3e-8 from zero and this path's fp32 sum at
    that element is exactly 0.0: one flip, 6e-3 of the largest v_conv gradient and 1e-2 of the q_lin gradients, while the logits agree to
    7e-8 and every gradient the flip does not reach to 3e-6 (forward_shared under that seed lands on the oracle's side of the same element).  That comparison
    judges a coin toss, not the arithmetic.  So the forward draws its seed under torch.manual_seed(1366): the first of
    0, 1, 2, ... for which the float64 ORACLE's own pre-activations (tests/feature_dropout_ref.relu_margins: no value of the
    code under test enters) keep the margins asserted below -- 3e-7 in the attention stage (the bound above), 1e-6 for the
    4 x 1024 classifier pre-activations (2560 terms of magnitude 0.1: 51 x 2^-24 x 0.1 = 3e-7).  Seeds 0 .. 1365 do not."""
    from oracle import vqa_oracle as O
    from tests.feature_dropout_ref import relu_margins
    meta, cfg, batch, _ = _full224_case()
    v, q, ql, a_idx, a_val = batch
    image_index = torch.tensor([1, 0, 0, 1])
    torch.manual_seed(meta["seed"])
    m = build(cfg, meta["V"]).train()
    sd64 = {k: t.detach().cpu().double() for k, t in m.state_dict().items()}
    feats = _encode(m, v, with_vprime=False)
    torch.manual_seed(FULL224_TORCH_SEED)
    y, loss, grads = step(m, feats, q, ql, a_idx, a_val, image_index, image_dropout=True)
    masks = bank_masks(m, m._last_ctx, feats, image_index, q.shape[1])
    assert masks["image"] is not None and masks["image"].shape[0] == 4
    # on the CPU, from the oracle alone: the case is one on which gradients can be compared
    pooled = O.image_encoder(sd64, v.double(), cfg["image"]["stride"])
    att_margin, cls_margin = relu_margins(sd64, cfg, pooled, image_index, q, ql, masks)
    print(f"[image-drop] full224: the oracle's ReLU pre-activation nearest to zero: attention {att_margin:.3e}, "
          f"classifier {cls_margin:.3e}")
    assert att_margin >= ATT_MARGIN and cls_margin >= CLS_MARGIN
    y_ref, loss_ref, g_ref = O.loss_and_grads(sd64, cfg, v.double()[image_index], q, ql, a_idx, a_val, masks=masks)
    err = float((y.cpu().double() - y_ref).abs().max())
    print(f"[image-drop] full224 train logits max abs err {err:.3e}; loss {float(loss):.6f} vs {float(loss_ref):.6f}")
    assert err < 1e-3
    assert abs(float(loss) - float(loss_ref)) < 1e-4
    _check_grads("image-drop full224", grads, g_ref, 1e-3)


# ----------------------------------------------------------------------------- nothing else moved
def _seeded(m, *a, **kw):
    torch.manual_seed(77)
    return step(m, *a, **kw)


def test_flag_off_eval_mode_and_zero_rate_run_what_ran_before():
    g = Golden("tiny_plus")
    cfg = tiny_cfg(g.meta)
    m = build(cfg, g.meta["V"], g.sd).train()
    v, q, ql, a_idx, a_val = _bank_batch(g)
    feats = _encode(m, v, with_vprime=False)
    args = (feats, q, ql, a_idx, a_val, BANK_INDEX)
    plain = _seeded(m, *args)
    assert m._last_ctx.vn.data_ptr() == feats.vn.data_ptr() and m._last_ctx.img.tolist() == BANK_INDEX.tolist()
    _same(plain, _seeded(m, *args, image_dropout=False))
    _same(plain, _seeded(m, *args, False))                              # positional
    dropped = _seeded(m, *args, image_dropout=True)
    assert not torch.equal(dropped[0], plain[0])                        # ... and on, it is another function
    m.eval()
    plain = step(m, *args)
    _same(plain, step(m, *args, image_dropout=False))
    _same(plain, step(m, *args, image_dropout=True))
    assert m._last_ctx.vn.data_ptr() == feats.vn.data_ptr()
    with torch.no_grad():                                               # outside a grad context: the same logits either way
        assert torch.equal(m.forward_features(feats, q.to(DEV), ql.to(DEV), BANK_INDEX, image_dropout=True), plain[0])
    # image.dropout = 0, train mode, the same seed
    cfg0 = tiny_cfg(g.meta)
    cfg0["image"]["dropout"] = 0.0
    m0 = build(cfg0, g.meta["V"], g.sd).train()
    feats0 = _encode(m0, v, with_vprime=False)
    args0 = (feats0, q, ql, a_idx, a_val, BANK_INDEX)
    _same(_seeded(m0, *args0), _seeded(m0, *args0, image_dropout=True))
    assert m0._last_ctx.vn.data_ptr() == feats0.vn.data_ptr()


def test_float16_bank_with_image_dropout_has_the_bits_of_the_fp32_bank_holding_its_values():
    from dl_vqa_amd.train import run_batch_features
    g = Golden("tiny_mul")
    cfg = tiny_cfg(g.meta)
    m = build(cfg, g.meta["V"], g.sd).train()
    v, q, ql, a_idx, a_val = _bank_batch(g)
    f16 = _encode(m, v, with_vprime=False, dtype=torch.float16)
    f32 = f16.to(torch.float32)
    assert f16.vn.dtype == torch.float16 and f32.vn.dtype == torch.float32
    a = _seeded(m, f16, q, ql, a_idx, a_val, BANK_INDEX, image_dropout=True)
    b = _seeded(m, f32, q, ql, a_idx, a_val, BANK_INDEX, image_dropout=True)
    _same(a, b)
    assert not torch.equal(a[0], _seeded(m, f16, q, ql, a_idx, a_val, BANK_INDEX)[0])
    # one draw per training forward with the flag on, through run_batch_features as well; none in eval mode
    batch = (None, q, a_idx, a_val, g.t["a_len"][QSEL], torch.arange(7), ql)
    torch.manual_seed(5)
    rng = torch.get_rng_state()
    with torch.no_grad():
        l_on, _ = run_batch_features(m, batch, 12, f16, BANK_INDEX, image_dropout=True)
    after = torch.get_rng_state()
    torch.set_rng_state(rng)
    m._next_seed()
    assert torch.equal(torch.get_rng_state(), after)
    torch.manual_seed(5)
    with torch.no_grad():
        l_off, _ = run_batch_features(m, batch, 12, f16, BANK_INDEX)
    assert float(l_on) != float(l_off)
    m.eval()
    rng = torch.get_rng_state()
    with torch.no_grad():
        m.forward_features(f16, q.to(DEV), ql.to(DEV), BANK_INDEX, image_dropout=True)
    assert torch.equal(torch.get_rng_state(), rng)


if __name__ == "__main__":
    worst = {}
    for shape in SHAPES:
        for p in (0.3, 0.5):
            for p2 in (0.0, 0.3):
                for half in (False, True):
                    w = kernel_case(*shape, p, p2, half)
                    worst[shape] = max(worst.get(shape, 0.0), w)
    print("vqa_gather_rows_drop_norm / _f16, vn_out against float64 (bound: 16 x 2^-24 x |ref| per element)")
    for shape, w in worst.items():
        print(f"  (n, M, P, C) = {shape}: max |err| / |ref| = {w:.3f} x 2^-24")
    print(f"  all cases: {max(worst.values()):.3f} x 2^-24")
