"""Conv2d -> ReLU -> MaxPool2d(2,2) in every kernel family, bit for bit, on inputs whose arithmetic is exact.

tests/conv_lattice_ref.py draws image, weights, bias and pooled gradient from a dyadic lattice on which every product and
every partial sum is an fp32 value (and every operand a bf16 / fp16 value), so a kernel's result cannot depend on its
summation order, tile shape, split-K plan or chunking: each fp32 output must EQUAL the float64 closed form, each bf16 / fp16
output its round-to-nearest-even.  The images are piecewise constant: several per cent of the windows hold tied maxima or
a maximum of exactly zero, and the arg-max bytes are compared as bytes with the rule of include/vqa_hip.h -- the first strict
maximum in the order dy*2+dx, byte 4 and output 0 where the maximum is <= 0.  tests/test_conv_lattice_ref_cpu.py holds the
reference to float64 autograd and shows that it tells `>=` from `>` in either place.

Every backward kernel is fed the REFERENCE's bytes in the layout it reads, never a forward kernel's.  Every buffer that
dl_vqa_amd.ops allocates is poisoned first (NaN, 0xFF for bytes; the split-K workspace included), so an element a kernel
does not write, or a slab it reads without having written it, cannot compare equal.  One `[lattice]` line per case:
family, shape, windows, tied and zero-maximum windows, elements compared, mismatches (asserted to be 0).
"""
import pytest
import torch

from tests import conv_lattice_ref as L
from tests import gemm_lattice_ref as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32


class _PoisoningTorch:
    """`torch` as dl_vqa_amd.ops sees it during these tests: empty() returns NaN / 0xFF instead of whatever was there."""

    def __getattr__(self, name):
        return getattr(torch, name)

    @staticmethod
    def empty(*size, dtype=F32, device=None):
        t = torch.empty(*size, dtype=dtype, device=device)
        return t.fill_(0xFF) if dtype == torch.uint8 else t.fill_(NAN)


@pytest.fixture(autouse=True)
def ops(monkeypatch):
    from dl_vqa_amd import ops as _ops
    monkeypatch.setattr(_ops, "torch", _PoisoningTorch())
    monkeypatch.setattr(_ops, "_ws", {})                       # a fresh, poisoned workspace
    assert bool(torch.isnan(_ops.workspace(64, torch.device(DEV))).all())
    return _ops


@pytest.fixture
def knob(monkeypatch):
    """Set a VQA_* knob for one test (the library reads them once: vqa_reload_knobs after every change and after the
    test's environment has been restored) -- the fixture of tests/test_kernels_gpu.py."""
    from dl_vqa_amd import _lib

    def set_knob(name, value):
        monkeypatch.setenv(name, value)
        _lib.load().vqa_reload_knobs()
    yield set_knob
    monkeypatch.undo()
    _lib.load().vqa_reload_knobs()


def dev(t, dtype=F32):
    """an exact copy of a float64 lattice tensor on the device in the kernel's operand type"""
    c = t.to(dtype)
    assert torch.equal(c.double(), t)
    return c.contiguous().to(DEV)


def poisoned(*shape, dtype=F32):
    return torch.full(shape, 0xFF if dtype == torch.uint8 else NAN, dtype=dtype, device=DEV)


class Tally:
    """Exact comparisons of one case; prints the case's [lattice] line and fails after it if anything differed."""

    def __init__(self, family, key, note="", lattice="bf16"):
        self.family, self.key, self.note, self.lattice, self.n, self.bad, self.where = family, key, note, lattice, 0, 0, []

    def eq(self, name, got, want):
        """got (device, any kernel output type) == want; a float64 reference is narrowed to got's type by round-to-nearest-even"""
        torch.cuda.synchronize()
        got = got.detach().cpu()
        if want.dtype == torch.float64 and got.dtype != torch.float64:
            want = {F32: L.rne_f32, BF16: L.rne_bf16, F16: L.rne_fp16}[got.dtype](want)
        want = want.detach().cpu()
        assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, want.shape, got.dtype, want.dtype)
        ne = got != want                                           # NaN (an unwritten element) differs from everything
        self.n += got.numel()
        if not torch.equal(got, want):
            self.bad += int(ne.sum())
            first = [int(v) for v in ne.nonzero()[0]]
            self.where.append(f"{name}: {int(ne.sum())} of {got.numel()} differ, first at {first}: "
                              f"got {got[tuple(first)].item()} want {want[tuple(first)].item()}")

    def done(self):
        s = L.cached_stats(*self.key, lattice=self.lattice)
        n = s["windows"]
        print(f"[lattice] {self.family} lattice={self.lattice} B,Ci,H,W,Co,ks,stride={self.key}{self.note}: windows {n} tied {round(s['tied'] * n)} "
              f"zero-max {round(s['zero_max'] * n)} compared {self.n} mismatches {self.bad}")
        assert self.bad == 0 and not self.where, "\n".join(self.where)


def nhwc_ref(ref, CiP=None):
    """the reference in the kernels' NHWC layouts: pooled, bytes, dX (pad channels zero)"""
    return L.nhwc(ref.pooled), L.nhwc(ref.argmax), L.nhwc(ref.dx, CiP)


# ----------------------------------------------------------------------------- fp32 implicit GEMM
def run_fp32(ops, shape, note=""):
    B, H, W, Ci, Co, stride = shape
    k = L.key(*shape)
    case, ref = L.cached(*k)
    CiP = (Ci + 3) // 4 * 4
    pooled_r, amax_r, dx_r = nhwc_ref(ref, CiP)
    t = Tally("fp32-igemm", k, note)
    xd, bd = dev(L.nhwc(case.x, CiP)), dev(case.b)
    wf, wd = ops.conv_pack_weights(dev(case.w), CiP)
    pooled, amax = ops.conv_fwd(xd, wf, bd, stride)
    t.eq("pooled", pooled, pooled_r)
    t.eq("arg-max bytes", amax, amax_r)
    dyd, am = dev(L.nhwc(case.dy)), amax_r.to(DEV)
    t.eq("dX (pad channels zero)", ops.conv_dgrad(dyd, am, wd, xd.shape, stride), dx_r)
    dw, db = poisoned(Co, Ci, 3, 3), poisoned(Co)
    ops.conv_wgrad(xd, dyd, am, dw, db, stride)
    t.eq("dW", dw, ref.dw)
    t.eq("dbias", db, ref.db)
    t.done()


@pytest.mark.parametrize("shape", L.FP32_CASES, ids=str)
def test_fp32_implicit_gemm(ops, shape):
    run_fp32(ops, shape)


@pytest.mark.parametrize("shape", L.KNOB_CASES, ids=str)
@pytest.mark.parametrize("name,value", [("VQA_BIG_TILES", "0"), ("VQA_BIG_TILES", "1"), ("VQA_BIG_TILES", "3"),
                                        ("VQA_PERSISTENT", "0"), ("VQA_PERSISTENT", "1"),
                                        ("VQA_WGRAD_192", "1"), ("VQA_WGRAD_384", "1")])
def test_fp32_implicit_gemm_forced_tiles(ops, knob, shape, name, value):
    """Every tile configuration, the persistent and the one-tile-per-workgroup kernels, the tall wgrad tiles: the same bits,
    dW included (its split-K plan changes with the tile; exact sums do not)."""
    knob(name, value)
    run_fp32(ops, shape, f" {name}={value}")


def test_fp32_implicit_gemm_batch_chunks(ops, knob):
    """VQA_CONV_CHUNK=2 walks B = 5 as 2 + 2 + 1 images; wgrad's chunks are further split-K slabs of one reduce"""
    knob("VQA_CONV_CHUNK", "2")
    run_fp32(ops, L.CHUNK_CASE, " VQA_CONV_CHUNK=2")


@pytest.mark.parametrize("forced", [False, True])
def test_fp32_forward_epilogue_staged_and_direct(ops, knob, forced):
    """Interior 128 x 128 tiles of the one-tile-per-workgroup kernel store through LDS in 16-byte pieces when pooled and
    arg-max are 16-byte aligned, and element by element otherwise.  ops.conv_fwd allocates its outputs (always aligned), so
    the entry point is called directly with views 0 and 1 elements into guarded buffers; forced: 128-row tiles, not
    persistent, whatever the size heuristics would choose."""
    from dl_vqa_amd import _lib
    if forced:
        knob("VQA_BIG_TILES", "0")
        knob("VQA_PERSISTENT", "0")
    shape = (2, 30, 30, 64, 128, 1)
    B, H, W, Ci, Co, stride = shape
    k = L.key(*shape)
    case, ref = L.cached(*k)
    pooled_r, amax_r, _ = nhwc_ref(ref)
    xd, bd = dev(L.nhwc(case.x)), dev(case.b)
    wf, _ = ops.conv_pack_weights(dev(case.w), Ci, need_wd=False)
    n = pooled_r.numel()
    t = Tally("fp32-igemm epilogue", k, f" forced={forced}")
    for off in (0, 1):
        pbuf, abuf = poisoned(n + 8), poisoned(n + 32, dtype=torch.uint8)
        pooled, amax = pbuf[4 + off:4 + off + n], abuf[16 + off:16 + off + n]
        assert (pooled.data_ptr() % 16 == 0) == (off == 0) and (amax.data_ptr() % 16 == 0) == (off == 0)
        _lib.call("vqa_conv3x3_relu_pool_fwd", xd.data_ptr(), wf.data_ptr(), bd.data_ptr(), pooled.data_ptr(), amax.data_ptr(),
                  B, H, W, Ci, Co, stride, 0, _lib.stream())
        t.eq(f"pooled (offset {off})", pooled.view(pooled_r.shape), pooled_r)
        t.eq(f"arg-max bytes (offset {off})", amax.view(amax_r.shape), amax_r)
        guard = torch.cat([pbuf[:4 + off], pbuf[4 + off + n:]])
        assert bool(torch.isnan(guard).all()), "pooled: a write outside the output"
        assert bool((torch.cat([abuf[:16 + off], abuf[16 + off + n:]]) == 0xFF).all()), "arg-max: a write outside the output"
    t.done()


# ----------------------------------------------------------------------------- first block (dedicated kernels)
def run_first_block(ops, shape):
    """conv0 forward in its five output modes from float and __half images, its two weight-gradient kernels and its
    backward-data kernel.  The bytes of every forward variant equal the reference's -- and so one another's and those of
    the generic kernel on nchw_to_nhwc4(x), which is run here as well: not one byte may differ."""
    B, Ci, H, W, Co = shape
    k = (B, Ci, H, W, Co, 3, 1)
    assert ops.conv0_supported(Ci, H, W, Co, 1) and ops.conv0_dgrad_supported(Ci, H, W, Co, 1)
    case, ref = L.cached(*k)
    pooled_r, amax_r, _ = nhwc_ref(ref)
    t = Tally("conv0", k)
    wdv, bd = dev(case.w), dev(case.b)
    for xdt in (F32, F16):
        xd = dev(case.x, xdt)
        tag = "fp16 image" if xdt == F16 else "fp32 image"
        p, a = ops.conv0_fwd(xd, wdv, bd)
        t.eq(f"{tag}: pooled fp32", p, pooled_r)
        t.eq(f"{tag}: bytes (fp32 out)", a, amax_r)
        p, a = ops.conv0_fwd(xd, wdv, bd, out_dtype=BF16)
        t.eq(f"{tag}: pooled bf16", p, pooled_r)
        t.eq(f"{tag}: bytes (bf16 out)", a, amax_r)
        p, a = ops.conv0_fwd(xd, wdv, bd, out_dtype=BF16, bf16_mfma=True)
        t.eq(f"{tag}: pooled bf16 MFMA", p, pooled_r)
        t.eq(f"{tag}: bytes (bf16 MFMA)", a, amax_r)
        p, a = ops.conv0_fwd(xd, wdv, bd, out_packed=True)
        torch.cuda.synchronize()
        assert p.dtype == BF16 and not bool(torch.isnan(p.float()).any())
        t.eq(f"{tag}: pooled x3-packed, unpacked", L.x3_unpack(p.cpu()), pooled_r)
        t.eq(f"{tag}: bytes (x3-packed out)", a, amax_r)
        p, a = ops.conv0_fwd(xd, wdv, bd, out_dtype=BF16, bf16_mfma=True, out_c16=True)
        t.eq(f"{tag}: pooled C16", p, L.to_c16(L.rne_bf16(pooled_r)))
        t.eq(f"{tag}: bytes (C16 out)", a, amax_r)
    wf, _ = ops.conv_pack_weights(wdv, 4, need_wd=False)
    p, a = ops.conv_fwd(ops.nchw_to_nhwc4(dev(case.x)), wf, bd, 1)
    t.eq("generic kernel on NHWC4: pooled", p, pooled_r)
    t.eq("generic kernel on NHWC4: bytes", a, amax_r)

    am, dy_r = amax_r.to(DEV), L.nhwc(case.dy)
    for xdt in (F32, F16):
        xd = dev(case.x, xdt)
        dw, db = poisoned(Co, Ci, 3, 3), poisoned(Co)
        ops.conv0_wgrad(xd, dev(dy_r), am, dw, db)
        t.eq(f"wgrad dW ({xdt})", dw, ref.dw)
        t.eq(f"wgrad dbias ({xdt})", db, ref.db)
        dw, db = poisoned(Co, Ci, 3, 3), poisoned(Co)
        ops.conv0_wgrad_bf16(xd, dev(dy_r, BF16), am, dw, db)
        t.eq(f"wgrad_bf16 dW ({xdt})", dw, ref.dw)
        t.eq(f"wgrad_bf16 dbias ({xdt})", db, ref.db)
    for dpt in (F32, BF16):
        for dvt in (F32, F16):
            dv = ops.conv0_dgrad(dev(dy_r, dpt), am, wdv, (B, Ci, H, W), out_dtype=dvt)
            t.eq(f"dgrad dP {dpt} -> dv {dvt}", dv, ref.dx)
    dv = ops.conv0_dgrad(dev(dy_r), am, wdv, (B, Ci, H, W), round_w_bf16=True)      # the lattice weights are bf16 values
    t.eq("dgrad with bf16-rounded weights", dv, ref.dx)
    t.done()


@pytest.mark.parametrize("shape", L.CONV0_CASES, ids=str)
def test_first_block(ops, shape):
    run_first_block(ops, shape)


def test_first_block_persistent_kernels_take_a_second_item(ops):
    """The C16 forward walks (image, block of 4 pooled rows) items on min(256 or 512, items) workgroups, the prefetching
    weight gradients walk pooled rows on min(512 or 768, rows): here every one of them has more work than workgroups, so the
    prefetch of the next item, the store of its registers and the compute in between run a second time.  dW and dbias sum
    257 * 100 pixels per weight; the lattice's budget still holds there (sum |a||b| = 5.6e4 < 2^22, asserted for this case in
    tests/test_conv_lattice_ref_cpu.py), so they are compared for equality like everything else."""
    B, Ci, H, W, Co = L.CONV0_PERSISTENT_CASE
    _, _, Hp, _ = L.out_hw(H, W, 3, 1)
    assert Hp == 5 and B * 2 > 512 and B * 5 > 768 and B * 5 > 512
    run_first_block(ops, L.CONV0_PERSISTENT_CASE)


# ----------------------------------------------------------------------------- fp32 on the bf16 matrix cores (x3)
def x3_plans(ops, shape):
    """ops.conv_x3_plan of the three passes: what the launchers decide for this layer and batch under the knobs in force"""
    B, H, W, Ci, Co, stride = shape
    return {p: ops.conv_x3_plan(p, B, H, W, Ci, Co, stride) for p in ("forward", "dgrad", "wgrad")}


def run_x3(ops, shape, lattice="bf16", note=""):
    """fp32 and x3-packed input, plain and packed output, dgrad from the fp32 and from the packed pooled gradient, wgrad with
    and without the packed pooled gradient, the bias gradient of x3_pack_pooled_grad; bytes and values equal the reference's,
    and those of the fp32 MFMA kernels run beside them in all three passes -- on a plane lattice these are fp32-exact,
    order-free values whose mid and lo planes are not zero: "fp32x3 = fp32", bit for bit.  The split and every packed tensor
    (x3_split of the packed weights; x3_pack of x, dy and the fp32 pooled output; the pooled tensor the packed epilogue
    writes; the packed gradient of x3_pack_pooled_grad) are compared PLANE BY PLANE with x3_planes: the sum of the planes
    alone would not notice a swapped mid and lo plane."""
    B, H, W, Ci, Co, stride = shape
    assert ops.conv_x3_supported(H, W, Ci, Co, stride) and not ops.conv_x3_supported(*L.X3_NOT_ADMITTED)
    k = L.key(*shape)
    case, ref = L.cached(*k, lattice=lattice)
    pooled_r, amax_r, dx_r = nhwc_ref(ref)
    t = Tally("fp32x3", k, note, lattice)
    xd, bd, dyd, am = dev(L.nhwc(case.x)), dev(case.b), dev(L.nhwc(case.dy)), amax_r.to(DEV)
    wf, wd = ops.conv_pack_weights(dev(case.w), Ci)
    wfx, wdx = ops.x3_split(wf), ops.x3_split(wd)
    torch.cuda.synchronize()
    for name, planes, packed in (("wf", wfx, wf), ("wd", wdx, wd)):
        for i, want in enumerate(G.x3_planes(packed.cpu().double())):
            t.eq(f"x3_split({name}): plane {i}", planes[i].double(), want)
    xp, dyp = ops.x3_pack(xd), ops.x3_pack(dyd)
    t.eq("x3_pack(x), unpacked", L.x3_unpack(xp.cpu()), L.nhwc(case.x))
    t.eq("x3_pack(x): planes", xp, L.x3_pack_planes(L.nhwc(case.x)))
    t.eq("x3_pack(dy): planes", dyp, L.x3_pack_planes(L.nhwc(case.dy)))
    t.eq("x3_pack(pooled): planes", ops.x3_pack(dev(pooled_r)), L.x3_pack_planes(pooled_r))
    p32, a32 = ops.conv_fwd(xd, wf, bd, stride)
    t.eq("fp32 MFMA: pooled", p32, pooled_r)
    t.eq("fp32 MFMA: bytes", a32, amax_r)
    t.eq("fp32 MFMA: dX", ops.conv_dgrad(dyd, am, wd, xd.shape, stride), dx_r)
    dw, db = poisoned(Co, Ci, 3, 3), poisoned(Co)
    ops.conv_wgrad(xd, dyd, am, dw, db, stride)
    t.eq("fp32 MFMA: dW", dw, ref.dw)
    t.eq("fp32 MFMA: dbias", db, ref.db)
    for name, xin in (("fp32 in", xd), ("packed in", xp)):
        p, a = ops.conv_fwd(xin, wfx, bd, stride, x3=True)
        t.eq(f"{name}: pooled", p, pooled_r)
        t.eq(f"{name}: bytes", a, amax_r)
        p, a = ops.conv_fwd(xin, wfx, bd, stride, x3=True, out_packed=True)
        torch.cuda.synchronize()
        assert not bool(torch.isnan(p.float()).any())
        t.eq(f"{name}: pooled packed, unpacked", L.x3_unpack(p.cpu()), pooled_r)
        t.eq(f"{name}: pooled packed: planes", p, L.x3_pack_planes(pooled_r))
        t.eq(f"{name}: bytes (packed out)", a, amax_r)
    t.eq("dgrad from fp32 dP", ops.conv_dgrad(dyd, am, wdx, xd.shape, stride, x3=True), dx_r)
    t.eq("dgrad from packed dP", ops.conv_dgrad(dyp, am, wdx, xd.shape, stride, x3=True), dx_r)
    db_s = poisoned(Co)
    dyp_s = ops.x3_pack_pooled_grad(dyd, am, db_s)
    t.eq("x3_pack_pooled_grad: packed dP, unpacked", L.x3_unpack(dyp_s.cpu()), L.nhwc(case.dy))
    t.eq("x3_pack_pooled_grad: planes", dyp_s, L.x3_pack_planes(L.nhwc(case.dy)))
    t.eq("x3_pack_pooled_grad: dbias", db_s, ref.db)
    for name, xin, packed_dp in (("fp32 in", xd, None), ("packed in", xp, None), ("packed in, packed dP", xp, dyp),
                                 ("fp32 in, packed dP", xd, dyp)):
        dw, db = poisoned(Co, Ci, 3, 3), poisoned(Co)
        ops.conv_wgrad(xin, dyd, am, dw, db, stride, x3=True, dpooled_packed=packed_dp)
        t.eq(f"wgrad {name}: dW", dw, ref.dw)
        t.eq(f"wgrad {name}: dbias", db, ref.db)
    dw = poisoned(Co, Ci, 3, 3)
    ops.conv_wgrad(xp, dyd, am, dw, None, stride, x3=True, dpooled_packed=dyp)        # dbias not asked for
    t.eq("wgrad packed in, packed dP, no dbias: dW", dw, ref.dw)
    t.done()


@pytest.mark.parametrize("shape", L.X3_CASES, ids=str)
def test_fp32x3(ops, shape):
    """The exact three-way bf16 split of a lattice value is (value, 0, 0): the six partial products are exact too, and five of
    them are zero.  Everything run_x3 runs; test_fp32x3_planes feeds the other five."""
    run_x3(ops, shape)


# shape -> (forward tile, dgrad tile and waves)
PLANE_TILES = {(2, 36, 36, 32, 64, 1): ((256, 64), (256, 64, 16)), (1, 36, 36, 96, 128, 1): ((192, 128), (192, 128, 8)),
               (2, 37, 67, 32, 64, 2): ((256, 64), (256, 64, 16))}


@pytest.mark.parametrize("lattice,shape", L.PLANE_CASES, ids=str)
def test_fp32x3_planes(ops, lattice, shape):
    """The plane lattices of tests/conv_lattice_ref.py: integers whose hi, mid and lo planes are occupied, every sum below 2^24,
    the three dropped plane products exactly zero -- each of the six kept products (hh, hm, mh, mm, hl, lh) reaches the
    result of each pass in some case here, and tests/test_conv_lattice_ref_cpu.py shows that leaving any one out changes at
    least a tenth of what is compared ([coverage]).  Forward on 256 x 64 and dgrad on the 16-wave 256 x 64 tile (32 -> 64
    channels), both on 192 x 128 (96 -> 128), asserted from the plan query; `iii` also at the stride-2 map."""
    plans = x3_plans(ops, shape)
    fwd, dgrad = PLANE_TILES[shape]
    assert (plans["forward"]["BM"], plans["forward"]["BN"]) == fwd, plans["forward"]
    assert (plans["dgrad"]["BM"], plans["dgrad"]["BN"], plans["dgrad"]["waves"]) == dgrad, plans["dgrad"]
    assert all(p["persistent"] == 0 and p["launches"] == 1 and p["chunk"] == shape[0] for p in plans.values()), plans
    run_x3(ops, shape, lattice, f" fwd {fwd[0]}x{fwd[1]} dgrad {dgrad[0]}x{dgrad[1]}/{dgrad[2]} waves")


@pytest.mark.parametrize("persistent", [1, 0])
@pytest.mark.parametrize("shape", L.X3_PERSISTENT_CASES, ids=str)
def test_fp32x3_persistent_kernels(ops, knob, shape, persistent):
    """More than 256 tiles: conv_fwd_x3_persistent_kernel and conv_dgrad_x3_persistent_kernel walk them on 256 workgroups (the
    loaders run ahead into the next tile during the epilogue); under VQA_PERSISTENT=0 the same tiles run one per workgroup.
    (4,114,114,96,128): forward 262, dgrad 271 tiles of 192 x 128; (6,114,114,64,64): forward 294, dgrad 305 tiles of 256 x 64.
    The bf16-exact lattice (ties and zero maxima included): the same bits either way."""
    if not persistent:
        knob("VQA_PERSISTENT", "0")
    plans = x3_plans(ops, shape)
    tile = (192, 128) if shape[4] > 64 else (256, 64)
    for p in ("forward", "dgrad"):
        assert (plans[p]["BM"], plans[p]["BN"]) == tile and plans[p]["tiles"] > 256 and plans[p]["persistent"] == persistent, plans[p]
    run_x3(ops, shape, note=f" tiles fwd {plans['forward']['tiles']} dgrad {plans['dgrad']['tiles']} persistent={persistent}")


def test_fp32x3_batch_chunks_with_packed_operands(ops, knob):
    """VQA_CONV_CHUNK=2 walks B = 5 as 2 + 2 + 1 images: the packed input, packed output and packed pooled gradient advance by
    6 bytes per element from chunk to chunk, wgrad's chunks are further split-K slabs of one reduce.  Lattice `iii` (its dW
    budget holds over the five images with fewer pooled gradients kept: conv_lattice_ref.PLANE_ARGS)."""
    knob("VQA_CONV_CHUNK", "2")
    plans = x3_plans(ops, L.X3_CHUNK_CASE)
    assert all(p["chunk"] == 2 and p["launches"] == 3 for p in plans.values()), plans
    run_x3(ops, L.X3_CHUNK_CASE, L.X3_CHUNK_LATTICE, " VQA_CONV_CHUNK=2")


# ----------------------------------------------------------------------------- bf16 implicit GEMM
def bf16_igemm_forward(ops, case, stride):
    B, Ci, H, W = case.x.shape
    xd = dev(L.nhwc(case.x), BF16)
    wfT, wdT = ops.conv_pack_weights_bf16(dev(case.w), Ci)
    p32, a32 = ops.conv_fwd_bf16(xd, wfT, dev(case.b), stride, out_dtype=F32)
    p16, a16 = ops.conv_fwd_bf16(xd, wfT, dev(case.b), stride)
    return xd, wdT, p32, a32, p16, a16


@pytest.mark.parametrize("shape", L.BF16_CASES, ids=str)
def test_bf16_implicit_gemm(ops, shape):
    B, H, W, Ci, Co, stride = shape
    k = L.key(*shape)
    case, ref = L.cached(*k)
    pooled_r, amax_r, dx_r = nhwc_ref(ref)
    t = Tally("bf16-igemm", k)
    xd, wdT, p32, a32, p16, a16 = bf16_igemm_forward(ops, case, stride)
    t.eq("pooled fp32", p32, pooled_r)
    t.eq("bytes (fp32 out)", a32, amax_r)
    t.eq("pooled bf16", p16, pooled_r)
    t.eq("bytes (bf16 out)", a16, amax_r)
    dyd, am = dev(L.nhwc(case.dy), BF16), amax_r.to(DEV)
    t.eq("dX fp32", ops.conv_dgrad_bf16(dyd, am, wdT, xd.shape, stride, out_dtype=F32), dx_r)
    t.eq("dX bf16", ops.conv_dgrad_bf16(dyd, am, wdT, xd.shape, stride), dx_r)
    dw, db = poisoned(Co, Ci, 3, 3), poisoned(Co)
    ops.conv_wgrad_bf16(xd, dyd, am, dw, db, stride)
    t.eq("dW", dw, ref.dw)
    t.eq("dbias", db, ref.db)
    t.done()


# ----------------------------------------------------------------------------- bf16 patch kernels (C16 layouts)
@pytest.mark.parametrize("shape", L.PCONV_CASES, ids=str)
def test_bf16_patch(ops, shape):
    """C16 activations and C16 bytes; the bytes, un-blocked, are also compared with the bf16 implicit-GEMM kernel's on the
    same input, directly.  Backward-data in its three output modes (where Ci % 64 == 0) and the weight gradient (where
    pconv_wgrad_supported) read the reference's bytes, channel-blocked."""
    B, H, W, Ci, Co = shape
    assert ops.pconv_supported(H, W, Ci, Co)
    k = L.key(*shape)
    case, ref = L.cached(*k)
    pooled_r, amax_r, dx_r = nhwc_ref(ref)
    t = Tally("bf16-patch", k)
    xd = dev(L.nhwc(case.x), BF16)
    xc = dev(L.to_c16(L.nhwc(case.x)), BF16)
    wf, wd = ops.pconv_pack_weights(dev(case.w), need_wd=Ci % 64 == 0)
    p32, a1 = ops.pconv_fwd(xc, wf, dev(case.b), Co, out_dtype=F32)
    p16, a2 = ops.pconv_fwd(xc, wf, dev(case.b), Co)
    t.eq("pooled fp32 NHWC", p32, pooled_r)
    t.eq("bytes C16 (fp32 out)", a1, L.to_c16(amax_r))
    t.eq("pooled bf16 C16", p16, L.to_c16(L.rne_bf16(pooled_r)))
    t.eq("bytes C16 (bf16 out)", a2, L.to_c16(amax_r))
    if Ci % 64 == 0:
        _, _, _, a_ig, _, _ = bf16_igemm_forward(ops, case, 1)
        t.eq("bytes, un-blocked, against the implicit-GEMM kernel's", L.from_c16(a1.cpu()), a_ig.cpu())
    dpc, amc = dev(L.to_c16(L.nhwc(case.dy)), BF16), L.to_c16(amax_r).to(DEV)
    if Ci % 64 == 0:
        t.eq("dX fp32 NHWC", ops.pconv_dgrad(dpc, amc, wd, xd.shape, out_dtype=F32), dx_r)
        t.eq("dX bf16 NHWC", ops.pconv_dgrad(dpc, amc, wd, xd.shape), dx_r)
        t.eq("dX bf16 C16", ops.pconv_dgrad(dpc, amc, wd, xd.shape, out_c16=True), L.to_c16(L.rne_bf16(dx_r)))
    if ops.pconv_wgrad_supported(H, W, Ci, Co):
        dw, db = poisoned(Co, Ci, 3, 3), poisoned(Co)
        ops.pconv_wgrad(xc, dpc, amc, dw, db)
        t.eq("dW", dw, ref.dw)
        t.eq("dbias", db, ref.db)
    t.done()


# ----------------------------------------------------------------------------- fp32 patch backward-data
@pytest.mark.parametrize("shape", L.PCONVF_CASES, ids=str)
def test_fp32_patch_dgrad(ops, shape):
    B, H, W, Ci, Co = shape
    assert ops.pconvf_supported(H, W, Ci, Co)
    k = L.key(*shape)
    case, ref = L.cached(*k)
    _, amax_r, dx_r = nhwc_ref(ref)
    t = Tally("fp32-patch dgrad", k)
    dyd, am, wdev = dev(L.nhwc(case.dy)), amax_r.to(DEV), dev(case.w)
    got = ops.pconvf_dgrad(dyd, am, ops.pconvf_pack_weights(wdev), (B, H, W, Ci))
    t.eq("dX", got, dx_r)
    _, wd = ops.conv_pack_weights(wdev, Ci)
    t.eq("dX against the implicit-GEMM kernel's", got, ops.conv_dgrad(dyd, am, wd, (B, H, W, Ci), 1).cpu())
    t.done()


# ----------------------------------------------------------------------------- kernel_size != 3 (materialised)
@pytest.mark.parametrize("shape", L.CONVK_CASES, ids=str)
def test_convk(ops, shape):
    """im2col + GEMM (bias in its epilogue) + pool / route / col2im: here the bias is added BEFORE the maximum is taken,
    which must not matter.  Run with the case's chunking and in one chunk: dW is the same sum, so the same bits."""
    B, H, W, Ci, Co, ks, stride, chunk = shape
    k = (B, Ci, H, W, Co, ks, stride)
    case, ref = L.cached(*k)
    CiP = (Ci + 3) // 4 * 4
    pooled_r, amax_r, dx_r = nhwc_ref(ref, CiP)
    xd, dyd, am = dev(L.nhwc(case.x, CiP)), dev(L.nhwc(case.dy)), amax_r.to(DEV)
    wk = ops.convk_pack_weights(dev(case.w), CiP)
    for ch in dict.fromkeys((chunk, 0)):
        t = Tally("convk", k, f" chunk={ch}")
        pooled, amax = ops.convk_fwd(xd, wk, dev(case.b), ks, stride, chunk=ch)
        t.eq("pooled", pooled, pooled_r)
        t.eq("arg-max bytes", amax, amax_r)
        dw, db = poisoned(Co, Ci, ks, ks), poisoned(Co)
        dx = ops.convk_bwd(xd, dyd, am, wk, dw, db, ks, stride, need_dx=True, chunk=ch)
        t.eq("dX (pad channels zero)", dx, dx_r)
        t.eq("dW", dw, ref.dw)
        t.eq("dbias", db, ref.db)
        t.done()
