"""Exact-arithmetic inputs and a float64 closed-form reference for Conv2d -> ReLU -> MaxPool2d(2,2).  No GPU, no HIP library.

The inputs live on a small dyadic lattice (image and pooled gradient: integers, weights and bias: multiples of 0.5), and
assert_exact bounds sum |a| |b| of every contraction below 2^22: every product and every partial sum, in any order, is then a
multiple of 0.5 below 2^22 in magnitude, which fp32 holds exactly (23 bits), and the operands themselves are exact in
bf16 / fp16.  A kernel's fp32 result therefore has to equal the float64 one bit for bit whatever its tiles, split-K plan or
chunking, and a bf16 / fp16 output its round-to-nearest-even.  The images are piecewise constant, so windows with tied
maxima and windows whose maximum is exactly zero are common, and the arg-max bytes can be compared as bytes with the rule
of include/vqa_hip.h: the first strict maximum in the order dy*2+dx wins; byte 4 and output 0 where the maximum (bias
included) is <= 0; floor in the convolution and in the pool.

tests/test_conv_lattice_ref_cpu.py checks this file against autograd; tests/test_conv_lattice_gpu.py judges the kernels.
"""
import functools
from collections import namedtuple

import torch
import torch.nn.functional as F

Case = namedtuple("Case", "x w b dy stride")            # x [B,Ci,H,W], w [Co,Ci,ks,ks], b [Co], dy [B,Co,Hp,Wp]; float64
Ref = namedtuple("Ref", "z pooled argmax dx dw db")      # NCHW float64; argmax uint8 NCHW

LIMIT = float(2 ** 22)


def out_hw(H, W, ks, stride):
    """(Ho, Wo, Hp, Wp): floor in the convolution, floor in the pool."""
    Ho, Wo = (H - ks) // stride + 1, (W - ks) // stride + 1
    return Ho, Wo, Ho // 2, Wo // 2


def lattice_case(B, Ci, H, W, Co, ks=3, stride=1, seed=0, tile=6, redraw=0.15, w_zero=0.5):
    """Image: integers in [-2, 2], constant per channel on tile x tile pixel tiles shifted by one pixel against the pool grid,
    then a fraction `redraw` of the pixel positions re-drawn (all channels of a pixel together).  Weights: multiples of 0.5 in
    [-1, 1], a fraction `w_zero` of them zeroed.  Bias: multiples of 0.5 in [-2, 2].  Pooled gradient: integers in [-3, 3]."""
    g = torch.Generator().manual_seed(seed)
    th, tw = (H + tile) // tile + 1, (W + tile) // tile + 1
    coarse = torch.randint(-2, 3, (B, Ci, th, tw), generator=g).double()
    x = coarse.repeat_interleave(tile, dim=2).repeat_interleave(tile, dim=3)[:, :, tile - 1:tile - 1 + H, tile - 1:tile - 1 + W]
    noise = torch.randint(-2, 3, (B, Ci, H, W), generator=g).double()
    mask = torch.rand(B, 1, H, W, generator=g) < redraw
    x = torch.where(mask, noise, x).contiguous()
    w = torch.randint(-2, 3, (Co, Ci, ks, ks), generator=g).double() * 0.5
    w = w * (torch.rand(Co, Ci, ks, ks, generator=g) >= w_zero).double()
    b = torch.randint(-4, 5, (Co,), generator=g).double() * 0.5
    _, _, Hp, Wp = out_hw(H, W, ks, stride)
    dy = torch.randint(-3, 4, (B, Co, Hp, Wp), generator=g).double()
    return Case(x, w, b, dy, stride)


def windows(z):
    """[B,Co,Ho,Wo] -> [B,Co,Hp,Wp,4], last index dy*2+dx; odd rows / columns dropped."""
    B, Co, Ho, Wo = z.shape
    Hp, Wp = Ho // 2, Wo // 2
    return z[:, :, :2 * Hp, :2 * Wp].reshape(B, Co, Hp, 2, Wp, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, Co, Hp, Wp, 4)


def unwindows(win, Ho, Wo):
    """inverse of windows(); the dropped rows / columns are zero"""
    B, Co, Hp, Wp, _ = win.shape
    out = torch.zeros(B, Co, Ho, Wo, dtype=win.dtype)
    out[:, :, :2 * Hp, :2 * Wp] = win.reshape(B, Co, Hp, Wp, 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, Co, 2 * Hp, 2 * Wp)
    return out


def pool_rule(z, tie_ge=False, alive_ge=False):
    """(pooled, argmax byte) of pre-activations z (bias included).  tie_ge / alive_ge are the two MUTANTS the tests must tell
    from the rule: a later equal value wins (>= for >), a window whose maximum is exactly 0 counts as alive (>= 0 for > 0)."""
    c = windows(z)
    best = c[..., 0].clone()
    a = torch.zeros(best.shape, dtype=torch.uint8)
    for k in (1, 2, 3):
        m = (c[..., k] >= best) if tie_ge else (c[..., k] > best)
        a = torch.where(m, torch.full_like(a, k), a)
        best = torch.where(m, c[..., k], best)
    alive = (best >= 0) if alive_ge else (best > 0)
    return torch.where(alive, best, torch.zeros_like(best)), torch.where(alive, a, torch.full_like(a, 4))


def route(dy, argmax, Ho, Wo):
    """the pre-pool gradient [B,Co,Ho,Wo]: dy where the byte names the pixel, zero elsewhere"""
    k = torch.arange(4, dtype=torch.uint8).view(1, 1, 1, 1, 4)
    return unwindows(torch.where(argmax.unsqueeze(-1) == k, dy.unsqueeze(-1), torch.zeros((), dtype=dy.dtype)), Ho, Wo)


def backward_from_bytes(case, argmax):
    """(dx, dw, db) of the block for GIVEN arg-max bytes, closed form"""
    x, w, b, dy, stride = case
    Ho, Wo, _, _ = out_hw(x.shape[2], x.shape[3], w.shape[2], stride)
    dz = route(dy, argmax, Ho, Wo)
    dx = torch.nn.grad.conv2d_input(x.shape, w, dz, stride=stride)
    dw = torch.nn.grad.conv2d_weight(x, w.shape, dz, stride=stride)
    return dx, dw, dz.sum(dim=(0, 2, 3))


def reference(x, w, b, dy, stride, tie_ge=False, alive_ge=False):
    z = F.conv2d(x, w, b, stride=stride)
    pooled, argmax = pool_rule(z, tie_ge, alive_ge)
    dx, dw, db = backward_from_bytes(Case(x, w, b, dy, stride), argmax)
    return Ref(z, pooled, argmax, dx, dw, db)


def on_lattice(t, step):
    return bool((t / step == torch.round(t / step)).all())


def assert_exact(case):
    """Raises unless every contraction of the forward pass, dX, dW and dbias stays on the 0.5 lattice below 2^22 in
    sum |a| |b| (dW and dbias summed over all B*Ho*Wo pixels, with |dy| at all four pixels of a window: whatever the routing)."""
    x, w, b, dy, stride = case
    if not (on_lattice(x, 1.0) and on_lattice(w, 0.5) and on_lattice(b, 0.5) and on_lattice(dy, 1.0)):
        raise AssertionError("operands off the lattice")
    Ho, Wo, _, _ = out_hw(x.shape[2], x.shape[3], w.shape[2], stride)
    dz = unwindows(dy.abs().unsqueeze(-1).expand(*dy.shape, 4), Ho, Wo)
    budgets = {
        "forward": float(F.conv2d(x.abs(), w.abs(), b.abs(), stride=stride).max()),
        "dX": float(torch.nn.grad.conv2d_input(x.shape, w.abs(), dz, stride=stride).max()),
        "dW": float(torch.nn.grad.conv2d_weight(x.abs(), w.shape, dz, stride=stride).max()),
        "dbias": float(dz.sum(dim=(0, 2, 3)).max()),
    }
    for name, v in budgets.items():
        if not v < LIMIT:
            raise AssertionError(f"{name}: sum |a||b| = {v} >= 2^22")
    return budgets


def tie_stats(case):
    """Fractions of the B*Co*Hp*Wp windows: tied (maximum > 0 reached by more than one pixel), zero_max (maximum exactly 0
    after the bias), dead, alive; of the tied ones: first_nonzero (the winner is not pixel 0) and later_tie (an equal value
    at a higher index than the winner: both `>=` and `last wins` then route differently)."""
    x, w, b, dy, stride = case
    c = windows(F.conv2d(x, w, b, stride=stride))
    best = c.max(dim=-1).values
    eq = c == best.unsqueeze(-1)
    first = (eq.cumsum(-1) == 0).sum(-1)                                # first / last index holding the maximum
    last = 3 - (eq.flip(-1).cumsum(-1) == 0).sum(-1)
    tied = (eq.sum(-1) > 1) & (best > 0)
    n, nt = best.numel(), max(int(tied.sum()), 1)
    return {"windows": n, "tied": int(tied.sum()) / n, "zero_max": int((best == 0).sum()) / n,
            "dead": int((best <= 0).sum()) / n, "alive": int((best > 0).sum()) / n,
            "first_nonzero": int((tied & (first != 0)).sum()) / nt, "later_tie": int((tied & (last > first)).sum()) / nt,
            "max_abs_z": float(c.abs().max())}


# ------------------------------------------------------------------------------------------------ layouts
def nhwc(t, cpad=None):
    """NCHW -> NHWC, channels zero-padded to cpad"""
    t = t.permute(0, 2, 3, 1)
    if cpad and cpad != t.shape[-1]:
        t = F.pad(t, (0, cpad - t.shape[-1]))
    return t.contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def to_c16(t_nhwc):
    """NHWC -> channel-blocked [B, C/16, H, W, 16] (activations and arg-max bytes of the patch kernels)"""
    B, H, W, C = t_nhwc.shape
    return t_nhwc.reshape(B, H, W, C // 16, 16).permute(0, 3, 1, 2, 4).contiguous()


def from_c16(t):
    B, Cb, H, W, _ = t.shape
    return t.permute(0, 2, 3, 1, 4).reshape(B, H, W, Cb * 16).contiguous()


def x3_unpack(p):
    """x3-packed [..., C/4, 3, 4] bf16 (hi[4] mid[4] lo[4] per four channels) -> float64 [..., C] = hi + mid + lo"""
    return p.double().sum(dim=-2).reshape(*p.shape[:-3], p.shape[-3] * 4)


def _rne(t, dtype):
    f = t.to(torch.float32)
    assert torch.equal(f.double(), t), "not an fp32 value: the narrowing would round twice"
    return f.to(dtype)


def rne_f32(t):
    """the fp32 copy of a float64 tensor; raises if a value is not an fp32 value"""
    return _rne(t, torch.float32)


def rne_bf16(t):
    """round-to-nearest-even of a float64 tensor of fp32-representable values to bf16"""
    return _rne(t, torch.bfloat16)


def rne_fp16(t):
    return _rne(t, torch.float16)


# ------------------------------------------------------------------------------------------------ the cases of the GPU file
# Shapes as the GPU tests name them.  Keys of cached() are (B, Ci, H, W, Co, ks, stride).
FP32_CASES = [      # B, H, W, Ci, Co, stride: fp32 implicit GEMM
    (3, 31, 29, 3, 8, 1),      # Ci = 3 padded to 4, odd sizes
    (2, 20, 20, 32, 32, 1),
    (2, 38, 42, 32, 96, 1),
    (2, 30, 30, 64, 128, 1),
    (1, 30, 34, 128, 256, 1),
    (2, 37, 41, 32, 64, 2),
    (3, 34, 70, 64, 64, 1),
]
KNOB_CASES = [(2, 30, 30, 64, 128, 1), (1, 30, 34, 128, 256, 1)]        # the 64 -> 128 and 128 -> 256 shapes, under forced tiles
CHUNK_CASE = (5, 26, 26, 32, 64, 1)                                     # VQA_CONV_CHUNK=2: 2 + 2 + 1 images
# B, Ci, H, W, Co; (2, 2, 13, 20, 64): Ci = 2, Hp = 5 (a one-row tail block), Wp = 9 (a partial 8-window tile)
CONV0_CASES = [(2, 3, 20, 24, 32), (3, 3, 31, 28, 64), (1, 1, 9, 12, 32), (1, 3, 14, 448, 64), (2, 2, 13, 20, 64)]
# More work than the persistent first-block kernels have workgroups, so each takes a second item: Hp = 5 is two row blocks
# per image for the C16 forward (grids of 256 and 512) and five pooled rows for the prefetching weight gradients (512 and
# 768); B = 257 is the smallest batch with 2 B > 512 (5 B > 768 holds from B = 154 on)
CONV0_PERSISTENT_CASE = (257, 3, 12, 12, 32)
# fp32x3 takes layers with 2 * Wp >= 32 only: at stride 2 the 41-wide map of FP32_CASES (Wp = 10) is not one of them, a
# 67-wide one (Wo = 33, Wp = 16: the narrowest admitted, with a dropped pool column) is
X3_CASES = [(2, 38, 42, 32, 96, 1), (2, 36, 36, 64, 128, 1), (2, 37, 67, 32, 64, 2)]
X3_NOT_ADMITTED = (37, 41, 32, 64, 2)                                   # H, W, Ci, Co, stride
BF16_CASES = [(2, 30, 30, 64, 128, 1), (1, 30, 34, 128, 256, 1), (2, 41, 37, 64, 128, 2)]
PCONV_CASES = [(2, 30, 30, 64, 128), (1, 30, 34, 128, 256), (3, 22, 20, 64, 64)]                  # B, H, W, Ci, Co
PCONVF_CASES = [(2, 30, 30, 64, 128), (3, 23, 41, 128, 256), (5, 17, 9, 64, 8), (1, 12, 200, 64, 16)]
CONVK_CASES = [(3, 23, 27, 3, 8, 5, 1, 2), (2, 33, 35, 8, 12, 2, 2, 1), (2, 17, 19, 16, 8, 1, 1, 0)]   # ..., ks, stride, chunk


def key(B, H, W, Ci, Co, stride=1, ks=3):
    return (B, Ci, H, W, Co, ks, stride)


def all_keys():
    """every case of tests/test_conv_lattice_gpu.py, once"""
    keys = [key(*c) for c in FP32_CASES + [CHUNK_CASE] + X3_CASES + BF16_CASES]
    keys += [(B, Ci, H, W, Co, 3, 1) for (B, Ci, H, W, Co) in CONV0_CASES + [CONV0_PERSISTENT_CASE]]
    keys += [key(*c) for c in PCONV_CASES + PCONVF_CASES]
    keys += [(B, Ci, H, W, Co, ks, stride) for (B, H, W, Ci, Co, ks, stride, _) in CONVK_CASES]
    return list(dict.fromkeys(keys))


def bf16_keys():
    """the cases whose operands the bf16 kernels read as bf16 (the x3 split of a bf16 value is the value itself)"""
    return list(dict.fromkeys([key(*c) for c in X3_CASES + BF16_CASES + PCONV_CASES] +
                              [(B, Ci, H, W, Co, 3, 1) for (B, Ci, H, W, Co) in CONV0_CASES + [CONV0_PERSISTENT_CASE]]))


# The default recipe with seed = H; small maps and few channels need more structure to reach the window counts that
# tests/test_conv_lattice_ref_cpu.py demands (100 tied, 50 zero-maximum windows): fewer re-drawn pixels, sparser weights.
OVERRIDES = {
    (1, 1, 9, 12, 32, 3, 1): dict(seed=2, redraw=0.05, w_zero=0.75),            # 480 windows
    (5, 64, 17, 9, 8, 3, 1): dict(seed=32, redraw=0.03, w_zero=0.985),          # 840 windows of 576 taps
    (3, 3, 23, 27, 8, 5, 1): dict(redraw=0.1),
}


def case_args(B, Ci, H, W, Co, ks=3, stride=1):
    return {"seed": H, **OVERRIDES.get((B, Ci, H, W, Co, ks, stride), {})}


@functools.lru_cache(maxsize=None)
def cached(B, Ci, H, W, Co, ks=3, stride=1):
    """(Case, Ref) of a shape, computed once per process and shared by the tests; treat as read-only"""
    case = lattice_case(B, Ci, H, W, Co, ks, stride, **case_args(B, Ci, H, W, Co, ks, stride))
    return case, reference(*case)


@functools.lru_cache(maxsize=None)
def cached_stats(*k):
    return tie_stats(cached(*k)[0])
