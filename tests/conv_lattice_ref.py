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

from tests import gemm_lattice_ref as G

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


# ------------------------------------------------------------------------------------------------ plane lattices (fp32x3)
# On the lattice above the exact three-way bf16 split of every operand is (value, 0, 0): of the six plane products the fp32x3
# kernels keep (hh, hm, mh, mm, hl, lh; csrc/x3_core.hpp) five are zero.  The plane lattices carry the recipe of
# tests/gemm_lattice_ref.py (digits 3*2^17, 3*2^8, 1: see its docstring; _three_planes and x3_planes are imported, the rule
# is stated there and nowhere else) over to the three passes of the block.  All values are integers (unit 1), every
# sum |a||b| stays below 2^24:
#   xi   x three planes, dense      w small, sparse           dy small, sparse          forward (x planes . w), dW (x planes . dz)
#   wi   x small, sparse            w three planes, dense     dy small, sparse          forward (x . w planes), dX (dz . w planes)
#   dyi  x in {-1,0,1}, 3 in 10     w +-1, sparse, bias -4    dy three planes, dense    dX (dz planes . w), dW (x . dz planes)
#        (few windows alive: see plane_case; dz, the routed dy, is what the contractions read)
#   iii  256 h + m, about half 0    256 h + m, thinned        256 h + m, thinned        all three: hh, hm, mh, mm
# "small": integers with 1 <= |v| <= 2 where not zero; bias: integers in [-4, 4].  A three-plane value is about 2^18.6, so the
# operand across from it may hold at most 42 in sum |b| per output element: the sparsity is dictated by the budget.  Where
# the sparse operand is the weights, the few non-zeros of a column are dealt tap by tap from permutations of the channels
# (_dealt), so that every row k of the contraction still meets a non-zero in some output column; a sparse pooled gradient is
# dealt over the windows in the same way (_spread), so that no 32-pixel K-step of the weight gradient is empty.
PLANE_LATTICES = ("xi", "wi", "dyi", "iii")
PAIRS = ("hh", "hm", "mh", "mm", "hl", "lh")             # the kept plane products: plane of A, plane of B
PASSES = ("forward", "dX", "dW")                         # A . B = x . w, dz . w, x . dz
LIMIT_X3 = G.LIMIT_X3


def _small(g, shape):
    """integers in {-2, -1, 1, 2}"""
    return (torch.randint(0, 2, shape, generator=g) * 2 - 1).double() * torch.randint(1, 3, shape, generator=g).double()


def _bernoulli(g, shape, p):
    return (torch.rand(shape, generator=g) < p).double()


def _spread(g, cols, rows, n):
    """[cols][rows] 0/1: n entries per column (fewer where two coincide), taken in order from back-to-back random permutations
    of the rows -- every row holds an entry in some column as soon as cols * n >= rows"""
    total = cols * n
    idx = torch.cat([torch.randperm(rows, generator=g) for _ in range(-(-total // rows))])[:total].view(cols, n)
    return torch.zeros(cols, rows, dtype=torch.float64).scatter_(1, idx, 1.0)


def _dealt(g, cols, chans, per):
    """[cols][chans][3][3] 0/1: for every tap, `per` channels per column dealt from permutations of the channels -- every
    column holds every tap, and every (channel, tap) is held by some column as soon as cols * per >= chans"""
    return torch.stack([_spread(g, cols, chans, per) for _ in range(9)], dim=2).view(cols, chans, 3, 3)


def _two_planes(g, shape):
    """256 h + m with h in {-1, 1} and m = h (three in five: 257 splits into 256 + 1), 0 or -h (one in five each: 256 and 255
    are bf16 values, one plane); uniform digits would leave the mid plane empty in seven of nine elements"""
    h = G._digits(g, shape, True)
    r = torch.rand(shape, generator=g)
    m = torch.where(r < 0.6, h, torch.where(r < 0.8, torch.zeros_like(h), -h))
    return 256 * h + m


DYI_ALIVE = 36      # 36 * (3 * 2^17 + 3 * 2^8 + 1) = 0.85 * 2^24


def plane_case(lattice, B, Ci, H, W, Co, stride=1, seed=0, iii_dy=320):
    """A case of one of the PLANE_LATTICES (the table above); ks = 3.  iii_dy: under `iii`, the pooled gradients kept per
    3 x 3 x Co patch (the dW budget grows with the number of pixels, so a larger batch keeps fewer)."""
    g = torch.Generator().manual_seed(seed * 7919 + PLANE_LATTICES.index(lattice))
    _, _, Hp, Wp = out_hw(H, W, 3, stride)
    nw = B * Hp * Wp
    xs, ws, ds = (B, Ci, H, W), (Co, Ci, 3, 3), (B, Co, Hp, Wp)
    per_window = lambda m: m.view(Co, B, Hp, Wp).permute(1, 0, 2, 3)                  # [Co][windows] -> [B,Co,Hp,Wp]
    if lattice == "xi":
        x = G._three_planes(g, xs)
        w = _small(g, ws) * _dealt(g, Co, Ci, max(2, -(-Ci // Co)))                   # 18 per output channel
        dy = _small(g, ds) * per_window(_spread(g, Co, nw, 20))                       # 20 windows per output channel
    elif lattice == "wi":
        x = _small(g, xs) * _bernoulli(g, xs, 10 / (9 * Ci))                          # about 10 per 3 x 3 x Ci patch
        w = G._three_planes(g, ws)
        dy = _small(g, ds) * _bernoulli(g, ds, 24 / (9 * Co))                         # a quarter of them per 3 x 3 x Co patch of dz
    elif lattice == "dyi":
        # dbias sums dy over a channel's alive windows and dW over their pixels, and at most 42 three-plane values fit below
        # 2^24.  dy stays dense (the pack kernels split every element of it); it is the FORWARD that leaves few windows of a
        # channel alive: x in {-1, 0, 1} with three in ten non-zero, 18 weights of +-1 per output channel (dealt, so that
        # every (input channel, tap) and every (output channel, tap) is held) and a bias of -4, so a window lives where five
        # more products are +1 than -1 -- some 17 to 75 windows of a channel.  dy is zero at all but DYI_ALIVE of a channel's
        # alive windows, drawn by lot: a hard cap, worth under 4 % of dy.
        x = G._digits(g, xs, True) * _bernoulli(g, xs, 0.3)
        w = G._digits(g, ws, True) * _dealt(g, Co, Ci, max(2, -(-Ci // Co)))
        b = torch.full((Co,), -4.0, dtype=torch.float64)
        alive = windows(F.conv2d(x, w, b, stride=stride)).max(dim=-1).values > 0          # [B,Co,Hp,Wp]
        lot = torch.where(alive.permute(1, 0, 2, 3).reshape(Co, nw), torch.rand(Co, nw, generator=g), torch.full((Co, nw), 2.0))
        rank = lot.argsort(dim=1).argsort(dim=1)                                          # alive windows first, in random order
        dy = G._three_planes(g, ds) * (~(alive & (per_window(rank) >= DYI_ALIVE))).double()
        return Case(x.contiguous(), w.contiguous(), b, dy.contiguous(), stride)
    elif lattice == "iii":
        x = _two_planes(g, xs) * _bernoulli(g, xs, 0.55)
        w = _two_planes(g, ws) * _bernoulli(g, ws, min(1.0, 150 / (9 * Ci)))
        dy = _two_planes(g, ds) * _bernoulli(g, ds, min(1.0, iii_dy / (9 * Co)))
    else:
        raise KeyError(lattice)
    b = torch.randint(-4, 5, (Co,), generator=g).double()
    return Case(x.contiguous(), w.contiguous(), b, dy.contiguous(), stride)


def _dropped_products(a, b):
    """max |mid_a| |lo_b| + |lo_a| |mid_b| + |lo_a| |lo_b|: zero iff the three products the kernels drop are zero for this pair"""
    _, ma, la = G.x3_planes(a)
    _, mb, lb = G.x3_planes(b)
    return float(ma.abs().max() * lb.abs().max() + la.abs().max() * mb.abs().max() + la.abs().max() * lb.abs().max())


def assert_exact_planes(case, argmax=None):
    """assert_exact for a plane case: integer operands, the three dropped plane products zero for the operand pair of every
    pass, and sum |a||b| < 2^24 in every contraction (|bias| included in the forward).  The backward budgets are taken with
    the reference's own routing, route(|dy|, argmax), not with |dy| at all four pixels of a window: every backward kernel of
    tests/test_conv_lattice_gpu.py is fed the reference's bytes, never a forward kernel's, so that routing is the only one a
    kernel under test can meet.  Returns the budgets."""
    x, w, b, dy, stride = case
    if not all(on_lattice(t, 1.0) for t in (x, w, b, dy)):
        raise AssertionError("operands off the lattice")
    Ho, Wo, _, _ = out_hw(x.shape[2], x.shape[3], w.shape[2], stride)
    if argmax is None:
        argmax = pool_rule(F.conv2d(x, w, b, stride=stride))[1]
    dz = route(dy, argmax, Ho, Wo)
    for name, (a, bb) in {"forward": (x, w), "dX": (dz, w), "dW": (x, dz)}.items():
        if _dropped_products(a, bb) != 0.0:
            raise AssertionError(f"{name}: a dropped plane product is not zero")
    budgets = {
        "forward": float(F.conv2d(x.abs(), w.abs(), b.abs(), stride=stride).max()),
        "dX": float(torch.nn.grad.conv2d_input(x.shape, w.abs(), dz.abs(), stride=stride).max()),
        "dW": float(torch.nn.grad.conv2d_weight(x.abs(), w.shape, dz.abs(), stride=stride).max()),
        "dbias": float(dz.abs().sum(dim=(0, 2, 3)).max()),
    }
    for name, v in budgets.items():
        if not v < LIMIT_X3:
            raise AssertionError(f"{name}: sum |a||b| = {v} >= 2^24")
    return budgets


def pass_operands(case, argmax, which):
    """(A, B) of a pass as the kernels contract them: forward x . w, dX dz . w, dW x . dz (dz: the routed pooled gradient)"""
    x, w, b, dy, stride = case
    Ho, Wo, _, _ = out_hw(x.shape[2], x.shape[3], w.shape[2], stride)
    dz = route(dy, argmax, Ho, Wo)
    return {"forward": (x, w), "dX": (dz, w), "dW": (x, dz)}[which]


def pair_terms(case, argmax, which):
    """{pair: the contraction of `which` with plane pair[0] of A and plane pair[1] of B} in float64, for the six kept pairs"""
    x, w, b, dy, stride = case
    a, bb = pass_operands(case, argmax, which)
    pa, pb = dict(zip("hml", G.x3_planes(a))), dict(zip("hml", G.x3_planes(bb)))
    contract = {"forward": lambda u, v: F.conv2d(u, v, None, stride=stride),
                "dX": lambda u, v: torch.nn.grad.conv2d_input(x.shape, v, u, stride=stride),
                "dW": lambda u, v: torch.nn.grad.conv2d_weight(u, w.shape, v, stride=stride)}[which]
    return {p: contract(pa[p[0]], pb[p[1]]) for p in PAIRS}


def pass_by_pairs(case, argmax, which, pairs, terms=None):
    """What tests/test_conv_lattice_gpu.py compares for a pass -- (pooled, bytes), (dX,) or (dW,) -- evaluated as the sum over
    the plane pairs in `pairs` only.  With all six PAIRS this is the reference; with one left out it is the MUTANT kernel that
    drops that product."""
    terms = terms or pair_terms(case, argmax, which)
    total = sum(terms[p] for p in pairs)
    if which == "forward":
        return pool_rule(total + case.b.view(1, -1, 1, 1))
    return (total,)


def empty_rows(case, argmax, which):
    """(rows, empty): the rows of the contraction of a pass -- each k of 9*Ci (forward: tap, input channel) or 9*Co (dX: tap,
    output channel), each K-step of 32 pixels m = (b, yo, xo) of the pool-covered conv output (dW, as the kernels walk it) --
    and how many of them hold only zeros of A for every output row or only zeros of B for every output column.  Such a row
    tests nothing."""
    x, w, b, dy, stride = case
    Ho, Wo, Hp, Wp = out_hw(x.shape[2], x.shape[3], 3, stride)
    dz = route(dy, argmax, Ho, Wo)
    tap = lambda ty, tx: x[:, :, ty:ty + stride * (2 * Hp - 1) + 1:stride, tx:tx + stride * (2 * Wp - 1) + 1:stride]
    if which == "forward":
        a = torch.stack([(tap(ty, tx) != 0).any(dim=3).any(dim=2).any(dim=0) for ty in range(3) for tx in range(3)], dim=1)
        live = a.view(-1, 3, 3) & (w != 0).any(dim=0)                               # [Ci,3,3]
    elif which == "dX":
        live = (dz != 0).any(dim=3).any(dim=2).any(dim=0).view(-1, 1, 1) & (w != 0).any(dim=1)      # [Co,3,3]
    else:
        steps = lambda t: F.pad(t, (0, 0, 0, -t.shape[0] % 32)).view(-1, 32 * t.shape[1]).ne(0).any(dim=1)
        pixels = lambda t: t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).double()    # [m][channels]
        xa = torch.stack([tap(ty, tx) != 0 for ty in range(3) for tx in range(3)]).any(dim=0)
        live = steps(pixels(xa)) & steps(pixels(dz[:, :, :2 * Hp, :2 * Wp]))
    return live.numel(), int((~live).sum())


def plane_occupancy(t):
    """shares of the elements whose hi / mid / lo plane is not zero, and in which all three are"""
    h, m, l = (p != 0 for p in G.x3_planes(t))
    share = lambda v: float(v.double().mean())
    return {"hi": share(h), "mid": share(m), "lo": share(l), "all": share(h & m & l)}


def x3_pack_planes(t_nhwc):
    """the x3-packed form [..., C/4, 3, 4] bf16 of a float64 NHWC tensor, built from x3_planes (hi[4] mid[4] lo[4] per four
    channels); raises if a plane is not a bf16 value"""
    out = []
    for p in G.x3_planes(t_nhwc):
        q = p.to(torch.bfloat16)
        assert torch.equal(q.double(), p), "a plane is not a bf16 value"
        out.append(q.reshape(*p.shape[:-1], p.shape[-1] // 4, 4))
    return torch.stack(out, dim=-2)


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


# fp32x3 on the plane lattices: forward on 256 x 64 and dgrad on the 16-wave 256 x 64 (Co = 64, Ci = 32), both on 192 x 128
# (Co = 128, Ci = 96); `iii` also at the narrowest admitted stride-2 map
PLANE_SHAPES = [(2, 36, 36, 32, 64, 1), (1, 36, 36, 96, 128, 1)]
PLANE_STRIDE2 = (2, 37, 67, 32, 64, 2)
PLANE_CASES = [(lat, s) for s in PLANE_SHAPES for lat in PLANE_LATTICES] + [("iii", PLANE_STRIDE2)]
# more than 256 tiles (the persistent forward / dgrad kernels), on the bf16-exact lattice: forward 262 and dgrad 271 tiles of
# 192 x 128, forward 294 and dgrad 305 tiles of 256 x 64
X3_PERSISTENT_CASES = [(4, 114, 114, 96, 128, 1), (6, 114, 114, 64, 64, 1)]
# VQA_CONV_CHUNK=2 with packed operands: 2 + 2 + 1 images, on lattice `iii` (the dW budget sums the pixels of all five
# images: PLANE_ARGS keeps fewer pooled gradients for it)
X3_CHUNK_CASE = (5, 38, 42, 64, 128, 1)
X3_CHUNK_LATTICE = "iii"
PLANE_ARGS = {("iii", (5, 64, 38, 42, 128, 3, 1)): dict(iii_dy=160)}


def key(B, H, W, Ci, Co, stride=1, ks=3):
    return (B, Ci, H, W, Co, ks, stride)


def plane_keys():
    """(lattice, key) of every plane case of tests/test_conv_lattice_gpu.py, once.  None of them is in all_keys() or
    bf16_keys(): their operands are not bf16 values."""
    return [(lat, key(*s)) for lat, s in PLANE_CASES + [(X3_CHUNK_LATTICE, X3_CHUNK_CASE)]]


def all_keys():
    """every case of tests/test_conv_lattice_gpu.py on the bf16-exact lattice, once"""
    keys = [key(*c) for c in FP32_CASES + [CHUNK_CASE] + X3_CASES + X3_PERSISTENT_CASES + BF16_CASES]
    keys += [(B, Ci, H, W, Co, 3, 1) for (B, Ci, H, W, Co) in CONV0_CASES + [CONV0_PERSISTENT_CASE]]
    keys += [key(*c) for c in PCONV_CASES + PCONVF_CASES]
    keys += [(B, Ci, H, W, Co, ks, stride) for (B, H, W, Ci, Co, ks, stride, _) in CONVK_CASES]
    return list(dict.fromkeys(keys))


def bf16_keys():
    """the cases whose operands the bf16 kernels read as bf16 (the x3 split of a bf16 value is the value itself)"""
    return list(dict.fromkeys([key(*c) for c in X3_CASES + X3_PERSISTENT_CASES + BF16_CASES + PCONV_CASES] +
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
def cached(B, Ci, H, W, Co, ks=3, stride=1, lattice="bf16"):
    """(Case, Ref) of a shape on a lattice ("bf16": the bf16-exact one, or one of PLANE_LATTICES; seed = H), computed once per
    process and shared by the tests; treat as read-only"""
    if lattice == "bf16":
        case = lattice_case(B, Ci, H, W, Co, ks, stride, **case_args(B, Ci, H, W, Co, ks, stride))
    else:
        assert ks == 3
        case = plane_case(lattice, B, Ci, H, W, Co, stride, seed=H, **PLANE_ARGS.get((lattice, (B, Ci, H, W, Co, ks, stride)), {}))
    return case, reference(*case)


@functools.lru_cache(maxsize=None)
def cached_stats(*k, lattice="bf16"):
    return tie_stats(cached(*k, lattice=lattice)[0])
