"""Exact-arithmetic operands, a float64 closed-form reference and the case table for vqa_gemm, vqa_gemm_x3, vqa_gemm_bf16 and
vqa_gemm_tall_bf16.  No GPU; the only use of the HIP library is by tests/test_gemm_lattice_ref_cpu.py, which asks it for each
case's plan.

Operands live on a dyadic lattice of bf16 values (A: integers in [-4, 4], B: multiples of 0.5 in [-2, 2] with about a third
zero, biases and row-group terms: multiples of 0.5 in [-2, 2], C0 of `accumulate`: integers in [-8, 8]).  assert_exact bounds
sum_k |a| |b| and then the epilogue's growth below 2^21: every partial sum in any order, every split-K slab and every epilogue
step is then a multiple of 0.25 below 2^21, which fp32 holds exactly, so the float64 result is the ONLY correct fp32 answer --
whatever the tile, the split-K plan or the reduce kernel -- and the only correct bf16 answer is its round-to-nearest-even.
This is a condition on the inputs, not a tolerance.

Every operand is stored as a view into a larger NaN-filled buffer (stored()): NaN between the row length and the leading
dimension, in GUARD_ROWS rows after the last valid one, before the 16-byte aligned start and in a tail.  An element a loader
does not mask poisons the output; an element an epilogue writes outside C shows as a NaN that is gone.

The x3 plane lattices keep vqa_gemm_x3 exact through its six kept plane products (hh, hm, mh, mm, hl, lh):
  (i)   A = 3*2^17 h + 3*2^8 m + l with h, m in {-1, 1}, l in {-1, 0, 1}, B integers in [-2, 2] (one plane), K = 16;
  (ii)  the mirror image: B has the three planes, A is integers in [-2, 2];
  (iii) A and B both 256 h + m with digits in {-1, 0, 1} (at most two planes each: the dropped products are zero), K <= 200.
The scales of (i) are not 2^16 : 2^8 : 1: under the round-to-nearest-even rule of vqa_x3_split a value such as
65536 + 256 + 1 = 65793 splits into 66048 - 255 + 0, two planes, and the lo plane -- the one the hl / lh products read -- would
stay empty.  With 3*2^17, 3*2^8 and 1 each digit is below half an ulp of the plane above it and the three planes are exactly
the three digits (x3_planes and the CPU tests check this against the rule).  Unit 1, limit 2^24.
"""
import functools
from collections import namedtuple

import torch

F32, X3, BF16, TALL = "vqa_gemm", "vqa_gemm_x3", "vqa_gemm_bf16", "vqa_gemm_tall_bf16"
LIMIT = float(2 ** 21)           # with unit 0.25: 23 bits
LIMIT_X3 = float(2 ** 24)        # plane lattices: unit 1
LEAD, TAIL, GUARD_ROWS = 16, 64, 2
NAN = float("nan")

# rg_div 0: no row-group term.  nbias: 0, 1 or 2 bias vectors.
Epi = namedtuple("Epi", "rg_div rg_op nbias relu accumulate aux", defaults=(0, 0, 0, False, False, False))
# knobs: ((name, value), ...) of VQA_* variables; plan: the fields of ops.gemm_plan the case is listed for;
# c_bf16: bf16 result; ldc: None = N + 3; c_off: elements added to C's aligned start; lattice: see operands();
# why: the mechanism a case of the tall engine is there for (tall_cases)
Case = namedtuple("Case", "group engine M N K transA transB knobs epi c_bf16 plan lattice ldc c_off why",
                  defaults=(False, True, (), Epi(), False, None, "std", None, 0, ""))
LAYOUTS = [(False, True), (False, False), (True, True), (True, False)]


def case_id(c):
    e = c.epi
    epi = "" if e == Epi() else f" rg{e.rg_div}{'*+'[e.rg_op == 0] if e.rg_div else ''} b{e.nbias}{' relu' * e.relu}{' acc' * e.accumulate}{' aux' * e.aux}"
    knobs = "".join(f" {k[4:]}={v}" for k, v in c.knobs)
    return (f"{c.engine[4:]} {c.M}x{c.N}x{c.K} {'T' if c.transA else 'N'}{'T' if c.transB else 'N'}{knobs}{epi}"
            f"{' bf16C' * c.c_bf16}{'' if c.lattice == 'std' else ' ' + c.lattice}{'' if c.ldc is None else f' ldc{c.ldc}'}{' off%d' % c.c_off if c.c_off else ''}")


# ------------------------------------------------------------------------------------------------ operands
def _half_steps(g, lo, hi, shape, nonzero=False):
    """multiples of 0.5 in [lo, hi]"""
    t = torch.randint(int(2 * lo), int(2 * hi) + 1, shape, generator=g).double() * 0.5
    if nonzero:
        t = torch.where(t == 0, torch.full_like(t, 1.5), t)
    return t


def _digits(g, shape, nonzero=False):
    return torch.randint(0, 2, shape, generator=g).double() * 2 - 1 if nonzero else torch.randint(-1, 2, shape, generator=g).double()


def _three_planes(g, shape):
    return 3 * 2.0 ** 17 * _digits(g, shape, True) + 3 * 2.0 ** 8 * _digits(g, shape, True) + _digits(g, shape)


@functools.lru_cache(maxsize=24)
def operands(lattice, M, N, K):
    """(A [M][K], B [K][N]) in float64, shared by every case of a shape; treat as read-only."""
    g = torch.Generator().manual_seed(M * 1000003 + N * 1009 + K)
    small = lambda shape: torch.randint(-2, 3, shape, generator=g).double()
    if lattice in ("std", "std16"):
        a = 16 if lattice == "std16" else 4                  # std16: outputs that bf16 cannot hold, and exact ties
        A = torch.randint(-a, a + 1, (M, K), generator=g).double()
        B = _half_steps(g, -2, 2, (K, N)) * (torch.rand(K, N, generator=g) >= 0.25).double()   # with the drawn zeros: a third
    elif lattice == "x3i":
        A, B = _three_planes(g, (M, K)), small((K, N))
    elif lattice == "x3ii":
        A, B = small((M, K)), _three_planes(g, (K, N))
    elif lattice == "x3iii":
        A = 256 * _digits(g, (M, K)) + _digits(g, (M, K))
        B = 256 * _digits(g, (K, N)) + _digits(g, (K, N))
    else:
        raise KeyError(lattice)
    return A, B


@functools.lru_cache(maxsize=24)
def product(lattice, M, N, K):
    A, B = operands(lattice, M, N, K)
    return A @ B


def extras(c):
    """bias1, bias2 [N], rowgroup [ceil(M / rg_div)][N], C0 [M][N] of a case (None where the case has none); only the tall
    engine's cases have a partial last group"""
    e = c.epi
    g = torch.Generator().manual_seed(c.M * 31 + c.N * 7 + e.rg_div)
    b1 = _half_steps(g, -2, 2, (c.N,)) if e.nbias >= 1 else None
    b2 = _half_steps(g, -2, 2, (c.N,)) if e.nbias >= 2 else None
    rg = None
    if e.rg_div:
        assert c.M % e.rg_div == 0 or c.engine == TALL, "M is a multiple of rg_div"
        rg = _half_steps(g, -2, 2, (-(-c.M // e.rg_div), c.N), nonzero=e.rg_op == 1)
    c0 = torch.randint(-8, 9, (c.M, c.N), generator=g).double() if e.accumulate else None
    return b1, b2, rg, c0


def epilogue(prod, e, b1, b2, rg, c0):
    """epi_apply (csrc/gemm_epilogue.hpp) in float64: row group with row // rg_div, biases, ReLU, + C0"""
    v = prod
    if e.rg_div:
        gx = rg[torch.arange(prod.shape[0]) // e.rg_div]
        v = v * gx if e.rg_op else v + gx
    if b1 is not None:
        v = v + b1
    if b2 is not None:
        v = v + b2
    if e.relu:
        v = torch.clamp_min(v, 0.0)
    if e.accumulate:
        v = v + c0
    return v


def expected(c):
    """(raw product = aux, result) in float64"""
    prod = product(c.lattice, c.M, c.N, c.K)
    return prod, epilogue(prod, c.epi, *extras(c))


def on_lattice(t, step):
    return t is None or bool((t / step == torch.round(t / step)).all())


def x3_planes(t):
    """vqa_x3_split's rule in float64: hi = RNE_bf16(x), mid = RNE_bf16(x - hi), lo = x - hi - mid"""
    rne = lambda v: v.float().to(torch.bfloat16).double()
    assert torch.equal(t.float().double(), t)
    hi = rne(t)
    mid = rne(t - hi)
    return hi, mid, t - hi - mid


@functools.lru_cache(maxsize=None)
def _operand_bound(lattice, M, N, K):
    """checks the operands of a shape against their lattice; returns an upper bound of sum_k |a_ik| |b_kj| over all i, j"""
    A, B = operands(lattice, M, N, K)
    plane = lattice.startswith("x3")
    if not (on_lattice(A, 1.0) and on_lattice(B, 1.0 if plane else 0.5)):
        raise AssertionError("operands off the lattice")
    if not plane:
        for t in (A, B):
            if not torch.equal(t.float().to(torch.bfloat16).double(), t):
                raise AssertionError("an operand is not a bf16 value")
    else:
        _, ma, la = x3_planes(A)                             # the three dropped products (mid*lo, lo*mid, lo*lo) are zero
        _, mb, lb = x3_planes(B)
        if float(ma.abs().max() * lb.abs().max() + la.abs().max() * mb.abs().max() + la.abs().max() * lb.abs().max()) != 0.0:
            raise AssertionError("a dropped plane product is not zero")
    # <= min(max_i sum_k |a_ik| * max |b|, max |a| * max_j sum_k |b_kj|)
    return min(float(A.abs().sum(1).max() * B.abs().max()), float(A.abs().max() * B.abs().sum(0).max()))


def assert_exact(c):
    """Raises unless the case meets the exactness condition of the module docstring; returns the bound it reached."""
    bound = _operand_bound(c.lattice, c.M, c.N, c.K)
    b1, b2, rg, c0 = extras(c)
    plane = c.lattice.startswith("x3")
    if not (on_lattice(b1, 0.5) and on_lattice(b2, 0.5) and on_lattice(rg, 0.5) and on_lattice(c0, 1.0)):
        raise AssertionError("epilogue operands off the lattice")
    e = c.epi
    if e.rg_div:
        bound = bound * float(rg.abs().max()) if e.rg_op else bound + float(rg.abs().max())
    bound += sum(float(t.abs().max()) for t in (b1, b2, c0) if t is not None)
    limit = LIMIT_X3 if plane else LIMIT
    if plane and (e != Epi() or c.engine != X3):
        raise AssertionError("plane lattices: plain vqa_gemm_x3 only")
    if not bound < limit:
        raise AssertionError(f"{case_id(c)}: bound {bound} >= {limit}")
    return bound


def rne_bf16(t):
    f = t.to(torch.float32)
    assert torch.equal(f.double(), t), "not an fp32 value: the narrowing would round twice"
    return f.to(torch.bfloat16)


def bf16_stats(t):
    """(share of the values that bf16 cannot hold, number of exact ties between two bf16 neighbours)"""
    f = t.to(torch.float32)
    unrep = float((f.to(torch.bfloat16).float() != f).double().mean())
    ties = int(((f.view(torch.int32) & 0xFFFF) == 0x8000).sum())
    return unrep, ties


# ------------------------------------------------------------------------------------------------ poisoned storage
def quantum(c):
    return 8 if c.engine in (BF16, TALL) else 4


def roundup(n, q):
    return (n + q - 1) // q * q


def stored(mat, rows, cols, ld, dtype, lead=LEAD):
    """A flat NaN buffer holding a [rows][cols] matrix with leading dimension ld at element `lead` (mat None: all NaN);
    GUARD_ROWS rows and TAIL elements follow.  body(flat, ...) is the [rows][cols] view, outside(flat, ...) the rest."""
    assert ld >= cols
    flat = torch.full((lead + (rows + GUARD_ROWS) * ld + TAIL,), NAN, dtype=dtype)
    if mat is not None:
        m = mat.to(dtype)
        assert mat.shape == (rows, cols) and torch.equal(m.double(), mat), "the stored copy is exact"
        body(flat, rows, cols, ld, lead).copy_(m)
    return flat


def body(flat, rows, cols, ld, lead=LEAD):
    return flat[lead:lead + rows * ld].view(rows, ld)[:, :cols]


def outside(flat, rows, cols, ld, lead=LEAD):
    """every element of the buffer that is not in the body, as integers (NaN payloads compare bit for bit)"""
    mask = torch.ones(flat.shape, dtype=torch.bool, device=flat.device)
    body(mask, rows, cols, ld, lead).fill_(False)
    return flat.view(torch.int32 if flat.dtype == torch.float32 else torch.int16)[mask]


def leading_dims(c):
    """(lda, ldb, ldc, rg_ld): every one longer than the row it holds"""
    if c.engine == TALL:                                     # multiples of 8 / 8 / 8 / 4, as the entry point asks
        return c.K + 8, c.K + 16, c.N + 8, c.N + 8
    q = quantum(c)
    lda = roundup(c.M if c.transA else c.K, q) + q
    ldb = roundup(c.K if c.transB else c.N, q) + q
    return lda, ldb, (c.N + 3 if c.ldc is None else c.ldc), c.N + 5


# ------------------------------------------------------------------------------------------------ the cases of the GPU file
ST1 = (("VQA_SPLIT_TARGET", "1"),)
TILE_KNOBS = {64: ST1, 128: ST1, 256: ST1 + (("VQA_BIG_TILES", "2"),)}


def _pers(v):
    return (("VQA_PERSISTENT", str(v)),)


def _even8(n, need):
    return roundup(n, 8) if need else n


def geometry_cases():
    """VQA_SPLIT_TARGET=1: 128 x 128 tiles, unsplit, at any M, N >= 128 with 16 or more K-steps; VQA_BIG_TILES=2 on top:
    256 x 128; VQA_PERSISTENT picks the kernel.  All-edge, all-interior and mixed tilings x K tails x layouts.  The bf16
    engine needs the row length of a reduction-major operand to be a multiple of 8: 130 -> 136, 300 -> 304, 260 -> 264."""
    out = []
    for M, N in ((130, 130), (256, 384), (300, 260)):
        for tA, tB in LAYOUTS:
            for K in (481, 512, 520, 545):
                for bm in (128, 256):
                    for p in (0, 1):
                        out.append(Case("geometry", F32, M, N, K, tA, tB, TILE_KNOBS[bm] + _pers(p),
                                        plan=dict(BM=bm, BN=128, splits=1, persistent=p)))
            for K in (1024, 1032, 1088):
                out.append(Case("geometry", BF16, _even8(M, tA), _even8(N, not tB), K, tA, tB, ST1,
                                plan=dict(BM=128, BN=128, splits=1), c_bf16=K == 1032))
            # 64 x 64 tiles, one launch: fewer than 16 K-steps
            out.append(Case("geometry", F32, M, N, 97, tA, tB, ST1, plan=dict(BM=64, BN=64, splits=1, persistent=0)))
            out.append(Case("geometry", BF16, _even8(M, tA), _even8(N, not tB), 200, tA, tB, ST1, plan=dict(BM=64, BN=64, splits=1)))
    return out


def real_plan_cases():
    """what the planner picks with no knob set (and, for tile order 1 without split-K, with VQA_SPLIT_TARGET=1)"""
    big = dict(BM=128, BN=128)
    out = [
        Case("real", F32, 1700, 1850, 72, plan=dict(big, tiles_m=14, tiles_n=15, splits=1, persistent=1)),
        Case("real", F32, 1700, 1850, 600, plan=dict(big, tiles_m=14, tiles_n=15, splits=1, persistent=0)),
        Case("real", F32, 1700, 1850, 2100, epi=Epi(nbias=1, relu=True), plan=dict(big, tiles_m=14, tiles_n=15, splits=2, persistent=0)),
        Case("real", F32, 136, 4000, 300, False, False, plan=dict(big, tiles_m=2, tiles_n=32, splits=2, order=1)),
        Case("real", BF16, 136, 4000, 640, False, True, plan=dict(big, tiles_m=2, tiles_n=32, splits=2, order=1)),
    ]
    # tile order 1 on the persistent kernel's tile walk and on one workgroup per tile: 2 (1) x 17 tiles, the last column ragged
    for bm in (128, 256):
        for p in (1, 0):
            out.append(Case("real", F32, 136, 2050, 512, p == 0, p == 1, TILE_KNOBS[bm] + _pers(p),
                            plan=dict(BM=bm, BN=128, tiles_n=17, splits=1, order=1, persistent=p)))
    for tA, tB in ((False, True), (True, False)):
        for p in (1, 0):
            out.append(Case("walk", F32, 2900, 2850, 40, tA, tB, _pers(p), plan=dict(big, tiles_m=23, tiles_n=23, splits=1, persistent=p)))
            out.append(Case("walk", F32, 2900, 2850, 40, tA, tB, (("VQA_BIG_TILES", "2"),) + _pers(p),
                            plan=dict(BM=256, BN=128, tiles_m=12, tiles_n=23, splits=1, persistent=p)))
    return out


def epilogue_cases():
    """Every gemm_epilogue_mode instantiation on every tile size, fp32 and bf16 C: rg_div around the tile height (BM - 1: the
    general mode, BM: one group per tile, BM + 1: a boundary that drifts through the tiles), 150 and 676 with a partial last
    tile; M = 2 rg_div; rg_ld > N; add and multiply; no, one, two biases; ReLU; accumulate; aux."""
    out = []
    flags = [dict(), dict(accumulate=True), dict(aux=True), dict(accumulate=True, aux=True)]
    for engine, bm, K in ((F32, 64, 97), (F32, 128, 512), (F32, 256, 520), (BF16, 64, 200), (BF16, 128, 1032)):
        knobs = TILE_KNOBS[bm] + (_pers(0) if engine == F32 and bm > 64 else ())
        plan = dict(BM=bm, BN=min(bm, 128), splits=1)
        i = 0
        for rg_div in (0, bm - 1, bm, bm + 1, 150, 676):
            for f in flags:
                M, N = (2 * rg_div if rg_div else 300), 136
                e = Epi(rg_div=rg_div, rg_op=i % 2, nbias=i % 3, relu=i % 4 < 2, **f)
                tA, tB = LAYOUTS[i % 4] if engine == F32 else (False, i % 2 == 0)
                out.append(Case("epilogue", engine, M, N, K, tA, tB, knobs, e, plan=plan))
                if engine == BF16 and not e.accumulate:
                    out.append(Case("epilogue", engine, M, N, K, tA, tB, knobs, e, c_bf16=True, plan=plan,
                                    lattice="std16"))
                i += 1
    # the persistent kernel runs the same epilogue after its tile walk
    out.append(Case("epilogue", F32, 258, 136, 512, False, True, ST1 + _pers(1), Epi(129, 1, 2, True, True, True),
                    plan=dict(BM=128, BN=128, splits=1, persistent=1)))
    out.append(Case("epilogue", F32, 514, 136, 512, True, False, TILE_KNOBS[256] + _pers(1), Epi(257, 0, 1, True, False, False),
                    plan=dict(BM=256, BN=128, splits=1, persistent=1)))
    return out


def staged_cases():
    """gemm_epilogue_bf16_staged: interior 128 x 128 tiles of vqa_gemm_bf16 with a bf16 C, 16-byte aligned, ldc % 8 == 0;
    1792 x 1920 is 14 x 15 interior tiles (210: the planner's own big-tile arm), 1704 x 1848 has edge tiles that go direct
    in the same launch.  Row groups of 128 (one per tile), 213 and 224 (boundaries inside tiles)."""
    big = dict(BM=128, BN=128, splits=1)
    out = []
    for M, N, divs in ((1792, 1920, (0, 128, 224)), (1704, 1848, (0, 213))):
        for i, d in enumerate(divs):
            e = Epi(rg_div=d, rg_op=i % 2, nbias=1 + i % 2, relu=i != 1)
            for ldc, off in ((N + 8, 0), (N + 3, 0), (N + 8, 1)):          # staged; ldc % 8 != 0 and a misaligned C: direct stores
                if (ldc, off) == (N + 8, 0) or (M, d) == (1792, 224):
                    out.append(Case("staged", BF16, M, N, 128, False, True, (), e, True, big, "std16", ldc, off))
    out.append(Case("staged", BF16, 1792, 1920, 128, True, False, (), Epi(224, 0, 2, True), True, big, "std16", 1928, 0))
    return out


def split_cases():
    """Split counts 2, 3, 4, 5, 9, 13, 14 and 52 through VQA_SPLIT_TARGET; N = 64: splitk_reduce4_kernel (four thread groups, two
    splits per trip plus a tail), N = 62: splitk_reduce_kernel.  K = 2049, 1921 and 2081 end in a K-step of one element that is
    alone in the last split (9 x 8, 13 x 5 and 14 x 5 K-steps cover 65, 61 and 66).  The epilogue flags are judged through the
    reduce kernels."""
    out = []
    epis = [Epi(), Epi(32, 1, 2, True, True, True), Epi(16, 0, 1, False, False, True), Epi(nbias=1, relu=True, accumulate=True)]
    for i, (K, target, splits, ks) in enumerate(((2100, 3, 3, 22), (2100, 5, 5, 14), (8200, 64, 52, 5), (2081, 2, 2, 33), (2081, 4, 4, 17),
                                                 (2049, 9, 9, 8), (1921, 13, 13, 5), (2081, 14, 14, 5))):
        for N in (64, 62):
            out.append(Case("split", F32, 64, N, K, i % 2 == 1, N == 64, (("VQA_SPLIT_TARGET", str(target)),), epis[i % 4],
                            plan=dict(BM=64, BN=64, splits=splits, ks_per_split=ks)))
    for i, (K, target, splits, ks) in enumerate(((2112, 3, 3, 11), (2120, 5, 5, 7), (8264, 13, 13, 10), (4168, 9, 9, 8))):
        for N, cb in ((64, False), (56, True), (62, False)):
            tA, tB = (i % 2 == 1, True) if N == 62 else LAYOUTS[(i + (N == 56)) % 4]       # N = 62 is no row length for [K][N]
            out.append(Case("split", BF16, 64, N, K, tA, tB, (("VQA_SPLIT_TARGET", str(target)),),
                            Epi(32, 0, 1, True) if cb else Epi(nbias=2, accumulate=True, aux=True), cb,
                            dict(BM=64, BN=64, splits=splits, ks_per_split=ks), "std16" if cb else "std"))
    # 128 x 128 tiles with split-K (the v_conv dW class): every split keeps 16 or more K-steps
    for tA, tB in LAYOUTS:
        out.append(Case("split", F32, 130, 132, 1569, tA, tB, (("VQA_SPLIT_TARGET", "12"),), Epi(65, 0, 1, True, False, True),
                        plan=dict(BM=128, BN=128, splits=3, ks_per_split=17)))
        out.append(Case("split", BF16, 136, 136, 5128, tA, tB, (("VQA_SPLIT_TARGET", "20"),), Epi(nbias=1),
                        plan=dict(BM=128, BN=128, splits=5, ks_per_split=17)))
    return out


def wide_cases():
    """plan_gemm_wide: bf16, A stored [K][M], B [K][N], N = 256, K >= 65536 -- admitted where the ordinary plan's workspace holds
    its slabs (128 rows: 64 splits either way), refused where it does not (256 rows); the test asserts whichever the query
    reports for the workspace it passes."""
    return [Case("wide", BF16, 128, 256, 65536, True, False, epi=Epi(nbias=1), plan=dict(splits=64)),
            Case("wide", BF16, 256, 256, 65536, True, False, plan=dict())]


def x3_cases():
    """vqa_gemm_x3 (192 x 128 tiles): the bf16-exact lattice (its mid and lo planes are zero) through one launch, split-K and
    the persistent kernel (more than 256 tiles), then the three plane lattices per layout."""
    out = []
    for tA, tB in LAYOUTS:
        out.append(Case("x3", X3, 200, 130, 97, tA, tB, plan=dict(BM=192, BN=128, tiles_m=2, tiles_n=2, splits=1, persistent=0)))
        out.append(Case("x3", X3, 200, 132 if tA else 130, 1001, tA, tB, epi=Epi(100, 1, 2, True, True, True),   # both reduce kernels
                        plan=dict(BM=192, BN=128, splits=4, ks_per_split=8, persistent=0)))
        for lat, K in (("x3i", 16), ("x3ii", 16), ("x3iii", 200)):
            out.append(Case("x3", X3, 200, 130, K, tA, tB, lattice=lat, plan=dict(BM=192, BN=128)))
    for rg_div, f in ((0, dict()), (191, dict()), (192, dict()), (193, dict(accumulate=True)), (0, dict(aux=True))):
        out.append(Case("x3", X3, 2 * rg_div if rg_div else 200, 130, 97, epi=Epi(rg_div, 0, 1, True, **f),
                        plan=dict(BM=192, BN=128, splits=1, persistent=0)))
    for p in (1, 0):
        for tA, tB in (LAYOUTS if p else LAYOUTS[::3]):
            out.append(Case("x3walk", X3, 3254, 2042, 40, tA, tB, _pers(p) if p == 0 else (), Epi(nbias=1),
                            plan=dict(BM=192, BN=128, tiles_m=17, tiles_n=16, splits=1, persistent=p)))
    return out


# ------------------------------------------------------------------------------------------------ the tall bf16 engine
TALL128 = (("VQA_TALL_BM", "128"),)


def tall_cases():
    """vqa_gemm_tall_bf16 (csrc/gemm_tall_bf16.hip) on the std16 lattice, A [M][K] . W [N][K]^T, bf16 C.  `plan` holds the fields
    of ops.gemm_tall_bf16_plan the case is listed for, `why` names its mechanism (tests/test_gemm_lattice_ref_cpu.py asserts
    it from the plan).  256-row tiles run on min(tiles, 256) workgroups, 128-row tiles (VQA_TALL_BM=128) on min(tiles, 512);
    workgroup w walks tiles w, w + grid, ... and prefetches across the seams; the row-group table of a tile is loaded at
    k-stage nk - 3 and stored at nk - 2, so K = 192 (nk = 3) is the minimum lead."""
    def case(why, M, N, K, rg_div=0, rg_op=0, relu=True, knobs=(), **plan):
        return Case("tall", TALL, M, N, K, False, True, knobs, Epi(rg_div, rg_op, 0, relu), True, dict(plan, nk=K // 64), "std16",
                    why=why)
    one = dict(BM=256, tiles_m=8, tiles_n=8, grid=64)
    seam = dict(tiles_m=34, tiles_n=8, grid=256)
    return [
        # one tile per workgroup
        case("nk1", 2048, 1024, 64, **one),
        case("nk1", 2048, 1024, 64, relu=False, **one),
        case("nk2", 2048, 1024, 128, **one),
        case("group-per-tile", 2048, 1024, 192, 256, 0, **one),
        case("one-group", 2048, 1024, 192, 2048, 1, relu=False, **one),
        # 272 tiles on 256 workgroups: 16 take a second tile, whose table is loaded in its first stage
        case("seam", 8700, 1024, 192, 300, 1, BM=256, **seam),
        # the training shape class: 13 images of 26 x 26 positions
        case("train", 8788, 1024, 256, 676, 0, relu=False, BM=256, tiles_m=35, tiles_n=8, grid=256),
        case("train", 8788, 1024, 256, 676, 0, BM=256, tiles_m=35, tiles_n=8, grid=256),
        # 15 images of 54 x 54 positions
        case("three-tiles", 43740, 384, 512, 2916, 1, BM=256, tiles_m=171, tiles_n=3, grid=256),
        case("odd-grid", 17000, 128, 64, relu=False, BM=256, tiles_m=67, tiles_n=1, grid=67),
        case("odd-grid", 17000, 128, 192, 1000, 0, BM=256, tiles_m=67, tiles_n=1, grid=67),
        case("partial-group", 8700, 1024, 256, 512, 0, BM=256, **seam),
        case("long-k", 2048, 1024, 1024, 1024, 0, relu=False, **one),
        # 128-row tiles
        case("seam", 8700, 1024, 192, 300, 1, knobs=TALL128, BM=128, tiles_m=68, tiles_n=8, grid=512),
        case("odd-grid", 17000, 128, 192, 1000, 0, knobs=TALL128, BM=128, tiles_m=133, tiles_n=1, grid=133),
        case("nk1", 2048, 1024, 64, knobs=TALL128, BM=128, tiles_m=16, tiles_n=8, grid=128),
    ]


def tall_cases_both_heights():
    """tall_cases(), and every 256-row case that is not already listed under VQA_TALL_BM=128 once more on 128-row tiles (the
    geometry restated here: 512 slots); the GPU file runs these, so every case is judged under both tile heights"""
    listed = tall_cases()
    have = {(c.M, c.N, c.K, c.epi) for c in listed if c.knobs}
    out = list(listed)
    for c in listed:
        if not c.knobs and (c.M, c.N, c.K, c.epi) not in have:
            tm, tn = -(-c.M // 128), c.N // 128
            out.append(c._replace(knobs=TALL128, plan=dict(BM=128, tiles_m=tm, tiles_n=tn, grid=min(tm * tn, 512), nk=c.K // 64)))
    return out


def tall_wrong_forms(c):
    """What four plausible bugs of the tall engine would compute for a case, in float64 before the bf16 rounding (the last one:
    after it): the row-group row taken as row // 256 (the tile, not the group), the last 64 of K left out, ReLU applied before
    the row-group term, and truncation to bf16 instead of round-to-nearest-even.  The CPU test shows that each differs from the
    expected output, so the case can see the bug."""
    A, B = operands(c.lattice, c.M, c.N, c.K)
    e, (_, _, rg, _) = c.epi, extras(c)
    prod = product(c.lattice, c.M, c.N, c.K)
    term = lambda v, gx: v * gx if e.rg_op else v + gx
    act = lambda v: torch.clamp_min(v, 0.0) if e.relu else v
    rows = torch.arange(c.M)
    tile_row = rg[torch.clamp(rows // 256, max=rg.shape[0] - 1)]
    want = expected(c)[1]
    trunc = (want.to(torch.float32).view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16)
    return {"group = row // 256": rne_bf16(act(term(prod, tile_row))),
            "last 64 of K dropped": rne_bf16(act(term(A[:, :c.K - 64] @ B[:c.K - 64], rg[rows // e.rg_div]))),
            "ReLU before the row-group term": rne_bf16(term(act(prod), rg[rows // e.rg_div])),
            "truncation to bf16": trunc}


@functools.lru_cache(maxsize=None)
def all_cases():
    cases = geometry_cases() + real_plan_cases() + epilogue_cases() + staged_cases() + split_cases() + wide_cases() + x3_cases()
    ids = [case_id(c) for c in cases]
    assert len(set(ids)) == len(ids), [i for i in ids if ids.count(i) > 1]
    return cases


def cases_of(*groups):
    return [c for c in all_cases() if c.group in groups]


def epilogue_instantiation(c, BM):
    """(RG, ACC, AUX) of the gemm_epilogue_mode instantiation gemm_epilogue picks"""
    e = c.epi
    rg = 0 if not e.rg_div else (1 if e.rg_div >= BM else 2)
    a, x = bool(e.accumulate), bool(e.aux)
    return (rg, a, x) if (rg, a, x) in ((0, False, False), (0, True, False), (1, False, False), (0, False, True)) else (rg, True, True)


def runs_staged(c, plan):
    """whether some tile of the case leaves through gemm_epilogue_bf16_staged (the test in gemm_bf16_kernel, csrc/bf16.hip)"""
    e = c.epi
    ldc = leading_dims(c)[2]
    return (c.engine == BF16 and c.c_bf16 and (plan["BM"], plan["BN"]) == (128, 128) and plan["splits"] == 1 and not e.aux and
            not e.accumulate and (not e.rg_div or e.rg_div >= 128) and c.M >= 128 and c.N >= 128 and ldc % 8 == 0 and c.c_off % 8 == 0)


def launch_form(plan):
    return "split-K" if plan["splits"] > 1 else "persistent" if plan["persistent"] else "plain"


def tile_name(plan):
    return "wide" if plan["wide"] else f"{plan['BM']}x{plan['BN']}"
