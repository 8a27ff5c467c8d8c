"""GPU: the gradient w.r.t. the input image (v.requires_grad) -- vqa_conv0_dgrad and vqa_nhwc_to_nchw against float64
torch, VqaNet's v.grad against the reference (tests/golden/input_grad*.npz) and the oracle on every form the first
block takes, the unchanged behaviour when v does not require grad, and the autograd contract."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.golden_util import GOLDEN, TINY_CASES, TRAIN_CASES, Golden, full_cfg, full_inputs, tiny_cfg
from tests.test_input_grad_cpu import reference_dv

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def rel(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-30)


def routed_dy(dp, am, H, W):
    """float64 dY [B,Co,H-2,W-2] routed from the NHWC pooled gradient through the arg-max bytes (4 = dead)."""
    B, Hp, Wp, Co = dp.shape
    dp, am = dp.double().permute(0, 3, 1, 2), am.long().permute(0, 3, 1, 2)
    dy = torch.zeros(B, Co, H - 2, W - 2, dtype=torch.float64, device=dp.device)
    for p in range(4):
        dy[:, :, p // 2:2 * Hp:2, p % 2:2 * Wp:2] = torch.where(am == p, dp, torch.zeros_like(dp))
    return dy


def dv_f64(dp, am, w, H, W):
    return F.conv_transpose2d(routed_dy(dp, am, H, W), w.double())


def random_inputs(B, H, W, Ci, Co, dtype, seed, dead=0.3):
    g = torch.Generator(device=DEV).manual_seed(seed)
    Hp, Wp = (H - 2) // 2, (W - 2) // 2
    dp = torch.randn(B, Hp, Wp, Co, device=DEV, generator=g).to(dtype)
    am = torch.randint(0, 4, (B, Hp, Wp, Co), device=DEV, generator=g, dtype=torch.uint8)
    am[torch.rand(B, Hp, Wp, Co, device=DEV, generator=g) < dead] = 4
    am[-1, : Hp // 3] = 4                                      # a band of dead windows
    w = torch.randn(Co, Ci, 3, 3, device=DEV, generator=g)
    return dp, am, w


# ------------------------------------------------------------------------------------------------ (a) kernel parity
@pytest.mark.parametrize("Ci", [1, 2, 3])
@pytest.mark.parametrize("Co", [32, 64])
@pytest.mark.parametrize("dp_dtype", [torch.float32, torch.bfloat16])
def test_conv0_dgrad_matches_float64(Ci, Co, dp_dtype):
    from dl_vqa_amd import ops
    B, H, W = 3, 37, 44                       # odd H: the last image row is reached by no pooled output
    assert ops.conv0_dgrad_supported(Ci, H, W, Co, 1)
    dp, am, w = random_inputs(B, H, W, Ci, Co, dp_dtype, seed=Ci * 100 + Co)
    dv = ops.conv0_dgrad(dp, am, w, (B, Ci, H, W))
    torch.cuda.synchronize()
    ref = dv_f64(dp, am, w, H, W)
    assert dv.shape == (B, Ci, H, W) and dv.dtype == torch.float32
    e = rel(dv, ref)
    print(f"[conv0_dgrad] Ci={Ci} Co={Co} dP {dp_dtype}: rel {e:.3e}")
    assert e <= 1e-6
    assert torch.all(dv[:, :, H - 1] == 0)                     # uncovered border: exact zeros
    # bf16-rounded weights (the bf16 path's choice)
    dvr = ops.conv0_dgrad(dp, am, w, (B, Ci, H, W), round_w_bf16=True)
    assert rel(dvr, dv_f64(dp, am, w.to(torch.bfloat16).float(), H, W)) <= 1e-6
    # fp16 output: the fp32 result rounded once
    dvh = ops.conv0_dgrad(dp, am, w, (B, Ci, H, W), out_dtype=torch.float16)
    torch.cuda.synchronize()
    assert dvh.dtype == torch.float16 and torch.equal(dvh, dv.half())
    # no atomics: bit-reproducible
    assert torch.equal(ops.conv0_dgrad(dp, am, w, (B, Ci, H, W)), dv)


def test_conv0_dgrad_all_windows_dead_gives_exact_zeros():
    from dl_vqa_amd import ops
    dp, am, w = random_inputs(2, 36, 40, 3, 64, torch.float32, seed=3)
    am.fill_(4)
    dv = ops.conv0_dgrad(dp, am, w, (2, 3, 36, 40))
    torch.cuda.synchronize()
    assert torch.all(dv == 0)


@pytest.mark.parametrize("out_dtype", [torch.float32, torch.float16])
def test_nhwc_to_nchw_is_the_permute(out_dtype):
    from dl_vqa_amd import ops
    for C, (B, H, W) in ((3, (2, 33, 35)), (4, (1, 8, 12)), (1, (3, 5, 7))):
        x = torch.randn(B, H, W, 4, device=DEV)
        y = ops.nhwc_to_nchw(x, C, out_dtype=out_dtype)
        torch.cuda.synchronize()
        assert torch.equal(y, x[..., :C].permute(0, 3, 1, 2).contiguous().to(out_dtype))


# ------------------------------------------------------------------------------------------------ (b) whole model
def build(cfg, V, sd=None, compute_dtype="fp32"):
    from dl_vqa_amd import VqaNet
    m = VqaNet(cfg, V, compute_dtype=compute_dtype)
    if sd is not None:
        m.load_state_dict(sd)
    return m.to(DEV)


def model_dv(m, v, q, ql, a_idx, a_val):
    from dl_vqa_amd.train import soft_ce_loss_and_score
    v = v.to(DEV).clone().requires_grad_(True)
    y = m(v, q.to(DEV), ql.to(DEV))
    loss, _ = soft_ce_loss_and_score(y, a_idx.to(DEV), a_val.to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    return v.grad, y


def oracle_dv(sd, cfg, v, q, ql, a_idx, a_val, masks=None, bf16=False):
    from oracle import vqa_oracle as O
    v = v.detach().cpu().float().clone().requires_grad_(True)
    logits = O.vqa_forward(sd, cfg, v, q.cpu(), ql.cpu(), masks=masks, bf16=bf16)
    (dv,) = torch.autograd.grad(O.soft_ce_loss(logits, a_idx.cpu(), a_val.cpu()), v)
    return dv


@pytest.mark.parametrize("name", TINY_CASES)
def test_golden_input_grad(name):
    g = Golden(name)
    m = build(tiny_cfg(g.meta), g.meta["V"], g.sd).eval()
    dv, _ = model_dv(m, g.t["v"], g.t["q"], g.t["q_len"], g.t["a_idx"], g.t["a_val"])
    assert m._last_ctx is not None and not m._last_ctx.fast0      # tiny fixtures: 8 output channels, the generic path
    e = rel(dv, reference_dv(name))
    print(f"[input-grad] {name}: {e:.3e}")
    assert dv.dtype == torch.float32 and dv.shape == g.t["v"].shape
    assert e <= 2e-4


@pytest.mark.parametrize("name", TRAIN_CASES)
def test_train_mode_input_grad_matches_oracle_with_shared_masks(name):
    from tests.hip_masks import hip_masks
    g = Golden(name)
    cfg = tiny_cfg(g.meta)
    m = build(cfg, g.meta["V"], g.sd).train()
    dv, _ = model_dv(m, g.t["v"], g.t["q"], g.t["q_len"], g.t["a_idx"], g.t["a_val"])
    ctx = m._last_ctx
    masks = hip_masks(m._engine, ctx.seed, g.t["v"].shape[0], g.t["q"].shape[1], ctx.acts[-1].shape[1], DEV)
    ref = oracle_dv(g.sd, cfg, g.t["v"], g.t["q"], g.t["q_len"], g.t["a_idx"], g.t["a_val"], masks=masks)
    e = rel(dv, ref)
    print(f"[input-grad] train {name}: {e:.3e}")
    assert e <= 2e-4


@pytest.mark.parametrize("compute_dtype", ["fp32", "fp32x3"])
def test_full224_input_grad(compute_dtype):
    g = Golden("full224_seed1")
    meta = g.meta
    torch.manual_seed(meta["seed"])
    cfg = full_cfg(meta["A"])
    m = build(cfg, meta["V"], compute_dtype=compute_dtype).eval()
    sd = {k: t.detach().cpu().clone() for k, t in m.state_dict().items()}
    v, q, ql, a_idx, a_val, _ = full_inputs(meta)
    dv, _ = model_dv(m, v, q, ql, a_idx, a_val)
    assert m._last_ctx.fast0                                  # the dedicated first block
    ref0 = torch.from_numpy(np.load(os.path.join(GOLDEN, "input_grad_full224.npz"))["dv0"])
    e_ref = rel(dv[0], ref0)
    e_or = rel(dv, oracle_dv(sd, cfg, v, q, ql, a_idx, a_val))
    print(f"[input-grad] full224 ({compute_dtype}): vs reference {e_ref:.3e}, vs oracle {e_or:.3e}")
    assert e_ref <= 2e-4 and e_or <= 2e-4


def small_dedicated_cfg():
    cfg = full_cfg(24)
    cfg["text"].update(question_features=32, embedding_features=20)
    cfg["image"]["num_channels"] = [3, 32, 64, 64]
    cfg["attention"]["hidden_dim"] = 48
    cfg["classifier"]["hidden_dim"] = 40
    return cfg


def test_small_dedicated_path_matches_oracle():
    from oracle import vqa_oracle as O
    cfg = small_dedicated_cfg()
    torch.manual_seed(3)
    m = build(cfg, 60).eval()
    sd = {k: t.detach().cpu().clone() for k, t in m.state_dict().items()}
    _, q, a_idx, a_val, _, _, ql = O.synthetic_batch(3, 36, 7, 60, 24, seed=5)
    v = torch.randn(3, 3, 36, 40, generator=torch.Generator().manual_seed(7))
    dv, _ = model_dv(m, v, q, ql, a_idx, a_val)
    assert m._last_ctx.fast0
    e = rel(dv, oracle_dv(sd, cfg, v, q, ql, a_idx, a_val))
    print(f"[input-grad] dedicated 36x40: {e:.3e}")
    assert e <= 2e-4


def test_bf16_configs3_architecture_matches_bf16_oracle(monkeypatch):
    """bf16 mode (configs[3]'s architecture, small image): the first block's backward-data reads the bf16 pooled gradient
    and uses the weights rounded to bf16, as the forward product does; the oracle's bf16 first block is patched to return
    the input gradient at the same rounding points."""
    from oracle import vqa_oracle as O
    from tests.hip_masks import hip_masks

    class FirstConvBf16WithInput(O._FirstConvBf16):
        @staticmethod
        def backward(ctx, gy):
            x, w = ctx.saved_tensors
            gw = torch.nn.grad.conv2d_weight(O.rb(x), w.shape, gy, stride=ctx.stride)
            gx = torch.nn.grad.conv2d_input(x.shape, O.rb(w), gy, stride=ctx.stride)
            return gx, gw, gy.sum(dim=(0, 2, 3)), None

    monkeypatch.setattr(O, "_FirstConvBf16", FirstConvBf16WithInput)
    cfg = full_cfg(1000)
    V, B, S, T = 3000, 2, 68, 6
    torch.manual_seed(4)
    m = build(cfg, V, compute_dtype="bf16").train()
    sd = {k: t.detach().cpu().clone() for k, t in m.state_dict().items()}
    v, q, a_idx, a_val, _, _, ql = O.synthetic_batch(B, S, T, V, 1000, seed=8)
    torch.manual_seed(9)
    dv, _ = model_dv(m, v, q, ql, a_idx, a_val)
    ctx = m._last_ctx
    masks = hip_masks(m._engine, ctx.seed, B, T, ctx.acts[-1].shape[1], DEV)
    ref = oracle_dv(sd, cfg, v, q, ql, a_idx, a_val, masks=masks, bf16=True)
    ref32 = oracle_dv(sd, cfg, v, q, ql, a_idx, a_val, masks=masks)
    e, dist = rel(dv, ref), rel(ref32, ref)
    print(f"[input-grad] bf16 configs[3] architecture: vs bf16 oracle {e:.3e}; bf16 vs fp32 oracle {dist:.3e}")
    assert e <= 2e-2


# ------------------------------------------------------------------------------------------------ (c) unchanged
@pytest.mark.parametrize("which", ["generic", "dedicated"])
def test_logits_and_parameter_grads_unchanged_by_v_requires_grad(which, monkeypatch):
    from dl_vqa_amd import ops
    from dl_vqa_amd.train import soft_ce_loss_and_score
    from oracle import vqa_oracle as O
    if which == "generic":
        g = Golden("tiny_plus")
        cfg, V, sd = tiny_cfg(g.meta), g.meta["V"], g.sd
        v, q, ql, a_idx, a_val = g.t["v"], g.t["q"], g.t["q_len"], g.t["a_idx"], g.t["a_val"]
    else:
        cfg, V = small_dedicated_cfg(), 60
        torch.manual_seed(3)
        sd = build(cfg, V).state_dict()
        v = torch.randn(3, 3, 36, 40, generator=torch.Generator().manual_seed(7))
        _, q, a_idx, a_val, _, _, ql = O.synthetic_batch(3, 36, 7, 60, 24, seed=5)
    calls = []
    for name in ("conv0_dgrad", "nhwc_to_nchw"):
        real = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a, _real=real, _n=name, **k: (calls.append(_n), _real(*a, **k))[1])
    out = {}
    for want in (False, True):
        m = build(cfg, V, sd).eval()
        vin = v.to(DEV).clone().requires_grad_(want)
        calls.clear()
        y = m(vin, q.to(DEV), ql.to(DEV))
        loss, _ = soft_ce_loss_and_score(y, a_idx.to(DEV), a_val.to(DEV))
        loss.backward()
        torch.cuda.synchronize()
        out[want] = (y.detach().clone(), {k: p.grad.clone() for k, p in m.named_parameters()}, list(calls))
    assert torch.equal(out[False][0], out[True][0])
    for k in out[False][1]:
        assert torch.equal(out[False][1][k], out[True][1][k]), k
    assert out[False][2] == []                                  # no new launch when v does not require grad
    assert out[True][2] == ["conv0_dgrad" if which == "dedicated" else "nhwc_to_nchw"]


# ------------------------------------------------------------------------------------------------ (d) contract
@pytest.mark.parametrize("which", ["generic", "dedicated"])
def test_fp16_image_gets_fp16_grad(which):
    from oracle import vqa_oracle as O
    if which == "generic":
        g = Golden("tiny_plus")
        m = build(tiny_cfg(g.meta), g.meta["V"], g.sd).eval()
        v, q, ql, a_idx, a_val = g.t["v"], g.t["q"], g.t["q_len"], g.t["a_idx"], g.t["a_val"]
    else:
        torch.manual_seed(3)
        m = build(small_dedicated_cfg(), 60).eval()
        v = torch.randn(3, 3, 36, 40, generator=torch.Generator().manual_seed(7))
        _, q, a_idx, a_val, _, _, ql = O.synthetic_batch(3, 36, 7, 60, 24, seed=5)
    v16 = v.half()
    dv16, _ = model_dv(m, v16, q, ql, a_idx, a_val)
    assert m._last_ctx.fast0 == (which == "dedicated")
    dv32, _ = model_dv(m, v16.float(), q, ql, a_idx, a_val)
    assert dv16.dtype == torch.float16 and dv16.shape == v.shape
    assert torch.equal(dv16, dv32.half())


@pytest.mark.parametrize("which", ["generic", "dedicated"])
def test_frozen_model_input_grad(which):
    from dl_vqa_amd.train import soft_ce_loss_and_score
    from oracle import vqa_oracle as O
    if which == "generic":
        g = Golden("tiny_mul")
        cfg, V, sd = tiny_cfg(g.meta), g.meta["V"], g.sd
        v, q, ql, a_idx, a_val = g.t["v"], g.t["q"], g.t["q_len"], g.t["a_idx"], g.t["a_val"]
    else:
        cfg, V = small_dedicated_cfg(), 60
        torch.manual_seed(3)
        sd = build(cfg, V).state_dict()
        v = torch.randn(3, 3, 36, 40, generator=torch.Generator().manual_seed(7))
        _, q, a_idx, a_val, _, _, ql = O.synthetic_batch(3, 36, 7, 60, 24, seed=5)
    m = build(cfg, V, sd).eval()
    dv_ref, _ = model_dv(m, v, q, ql, a_idx, a_val)
    m = build(cfg, V, sd).eval().requires_grad_(False)
    vin = v.to(DEV).clone().requires_grad_(True)
    m._ensure_flat()
    flat_before = m._flat_grad.clone()
    y = m(vin, q.to(DEV), ql.to(DEV))
    loss, _ = soft_ce_loss_and_score(y, a_idx.to(DEV), a_val.to(DEV))
    (dv,) = torch.autograd.grad(loss, vin)
    torch.cuda.synchronize()
    assert torch.equal(dv, dv_ref)
    assert all(p.grad is None for p in m.parameters())
    assert torch.equal(m._flat_grad, flat_before)
    # loss.backward() works too and fills v.grad only
    y = m(vin, q.to(DEV), ql.to(DEV))
    soft_ce_loss_and_score(y, a_idx.to(DEV), a_val.to(DEV))[0].backward()
    torch.cuda.synchronize()
    assert torch.equal(vin.grad, dv_ref) and all(p.grad is None for p in m.parameters())


def test_two_backward_passes_are_bit_identical():
    torch.manual_seed(3)
    m = build(small_dedicated_cfg(), 60).eval()
    from oracle import vqa_oracle as O
    v = torch.randn(3, 3, 36, 40, generator=torch.Generator().manual_seed(7))
    _, q, a_idx, a_val, _, _, ql = O.synthetic_batch(3, 36, 7, 60, 24, seed=5)
    d1, _ = model_dv(m, v, q, ql, a_idx, a_val)
    m.zero_grad()
    d2, _ = model_dv(m, v, q, ql, a_idx, a_val)
    assert torch.equal(d1, d2)


def test_four_channel_image_takes_the_generic_path():
    from oracle import vqa_oracle as O
    cfg = small_dedicated_cfg()
    cfg["image"]["num_channels"] = [4, 32, 64, 64]
    torch.manual_seed(6)
    m = build(cfg, 60).eval()
    sd = {k: t.detach().cpu().clone() for k, t in m.state_dict().items()}
    v = torch.randn(2, 4, 36, 40, generator=torch.Generator().manual_seed(8))
    _, q, a_idx, a_val, _, _, ql = O.synthetic_batch(2, 36, 7, 60, 24, seed=9)
    dv, _ = model_dv(m, v, q, ql, a_idx, a_val)
    assert not m._last_ctx.fast0
    e = rel(dv, oracle_dv(sd, cfg, v, q, ql, a_idx, a_val))
    print(f"[input-grad] 4-channel image (generic path): {e:.3e}")
    assert e <= 2e-4


# ------------------------------------------------------------------------------------------------ (e) scale
@pytest.mark.parametrize("B,S,dp_dtype", [(256, 224, torch.float32), (512, 448, torch.bfloat16)])
def test_conv0_dgrad_at_scale(B, S, dp_dtype):
    """configs[1] (fp32 pooled gradient) and configs[3] (bf16, 1.63 G elements: offsets beyond 2^31 bytes), 4 sampled images
    against float64 on the CPU."""
    from dl_vqa_amd import ops
    Ci, Co = 3, 64
    dp, am, w = random_inputs(B, S, S, Ci, Co, dp_dtype, seed=B)
    dv = ops.conv0_dgrad(dp, am, w, (B, Ci, S, S))
    torch.cuda.synchronize()
    for b in (0, 1, B // 2 + 1, B - 1):
        ref = dv_f64(dp[b:b + 1].cpu(), am[b:b + 1].cpu(), w.cpu(), S, S)
        e = rel(dv[b:b + 1], ref)
        print(f"[conv0_dgrad] B={B} S={S} image {b}: rel {e:.3e}")
        assert e <= 1e-6
    del dp, am, dv
    torch.cuda.empty_cache()
