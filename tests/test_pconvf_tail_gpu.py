"""fp32 patch backward-data (csrc/conv_patch_f32.hip): the right-sized last tile of an image and the carried epilogue
coordinates, bit for bit.

A tile of the kernel is a segment of SEG = 1024 (64-channel output) or 512 (128-channel output) positions of the padded-width
raster H * (W + 2); a wave owns NI row blocks of 32 positions, NI = 4 in every tile but an image's last one, where
NI = ceil(positions left / G) with G = 256 or 128.  The shapes below reach every NI of both configurations, the boundaries
between them (256 and 258 positions; 128 and 130), and images of one tile and of several; each case asserts the NI it is
there for, so the list cannot drift.  The MIXED cases are for the seams between tiles: a workgroup's stream takes the units
s, s + 256, ... of the B * segs units, the next tile's patch is routed a stage ahead and its operands are loaded two stages
ahead, each with the length of the tile it belongs to.  Their segment counts are odd (coprime with the 256 streams), so one
stream's units differ in segment, and the test computes every stream's unit list as the kernel does and asserts that full
tiles are followed by short ones and short ones by full ones (and, in the three-tile case, full - short - full).  The width
sweep is for the epilogue's (y, x), which are divided out once per tile and carried from element to element after that: rows
of 6 positions (the step of 5 wraps on nearly every element) up to rows of 258.

Inputs are the exact-arithmetic lattice of tests/conv_lattice_ref.py (|dX| terms: 9 Co products of at most 1 * 3, far below
2^22), so every fp32 output has to EQUAL the float64 closed form and the implicit-GEMM kernel's output, as in
test_conv_lattice_gpu.py::test_fp32_patch_dgrad.  The output is a NaN-poisoned slice in the middle of a larger NaN-poisoned
allocation: an element the kernel does not write differs from the reference, and a store in front of the tensor or past its
end leaves a number in a guard.
"""
import pytest
import torch

from tests import conv_lattice_ref as L
from tests.test_conv_lattice_gpu import DEV, NAN, Tally, dev, nhwc_ref, ops  # noqa: F401  (ops: the poisoning fixture)

pytestmark = pytest.mark.gpu
GUARD = 1 << 16                                            # floats in front of and behind the output

# (B, H, W, Ci, Co), NI of the last tile, tiles per image
TAIL_CASES = [
    ((1, 14, 14, 64, 8), 1, 1),          # 224 positions
    ((1, 20, 22, 64, 8), 2, 1),          # 480
    ((1, 24, 26, 64, 8), 3, 1),          # 672
    ((1, 30, 30, 64, 8), 4, 1),          # 960
    ((1, 16, 14, 64, 8), 1, 1),          # exactly 256
    ((1, 6, 41, 64, 8), 2, 1),           # 258
    ((2, 38, 38, 64, 16), 2, 2),         # one full tile, then 496 positions
    ((2, 111, 111, 64, 16), 1, 13),      # the benchmark raster: 12 full tiles and 255 positions
    ((130, 38, 38, 64, 8), 2, 2),        # 260 units on 256 streams: streams 0..3 walk two tiles, of the same segment (256 is even)
    ((1, 14, 14, 128, 8), 2, 1),         # 224 positions, SEG 512
    ((1, 16, 18, 128, 8), 3, 1),         # 320
    ((1, 18, 20, 128, 8), 4, 1),         # 396
    ((1, 20, 22, 128, 8), 4, 1),         # 480
    ((3, 23, 41, 128, 16), 4, 2),        # 512 + 477
    ((1, 8, 14, 128, 8), 1, 1),          # exactly 128: NI 1 of the 128-channel configuration
    ((1, 10, 11, 128, 8), 2, 1),         # 130
    ((2, 24, 22, 128, 8), 1, 2),         # 512 + 64: a full tile, then NI 1
]
# a stream walks tiles of different NI: odd segs, B * segs > 256
MIXED_CASES = [
    ((172, 46, 46, 64, 8), 1, 3),        # 2208 positions; 516 units: stream 1 walks segments 1, 2, 0 = NI 4, 1, 4
    ((87, 50, 48, 64, 16), 2, 3),        # 2500 positions, two K-slices per tile; 261 units
    ((87, 36, 36, 128, 8), 3, 3),        # 1368 positions of the 128-channel configuration; 261 units
]
STREAMS = 256                                              # workgroups of a launch (one slab of output channels in every case here)
SWEEP_WIDTHS = [4, 5, 6, 7, 9, 31, 62, 63, 64, 126, 127, 128, 200, 255, 256]


def tile_plan(H, W, Ci):
    """(tiles per image, NI of the last one) as the launcher computes them"""
    seg, gran = (512, 128) if Ci % 128 == 0 else (1024, 256)
    positions = H * (W + 2)
    segs = -(-positions // seg)
    valid_last = positions - (segs - 1) * seg
    return segs, -(-valid_last // gran)


def test_the_cases_reach_every_row_block_count_of_both_configurations():
    seen = {(Ci, tile_plan(H, W, Ci)[1]) for (_, H, W, Ci, _), _, _ in TAIL_CASES}
    assert seen == {(Ci, ni) for Ci in (64, 128) for ni in (1, 2, 3, 4)}
    several = {(Ci, tile_plan(H, W, Ci)[1]) for (_, H, W, Ci, _), _, segs in TAIL_CASES if segs > 1}
    assert {(64, 1), (64, 2), (128, 1), (128, 4)} <= several


def run_case(ops, shape):
    B, H, W, Ci, Co = shape
    assert ops.pconvf_supported(H, W, Ci, Co)
    assert 9 * Co * 1.0 * 3.0 < L.LIMIT                    # sum |w| |dy| of a dX element: exact in fp32 in any order
    k = L.key(*shape)
    case, ref = L.cached(*k)
    _, amax_r, dx_r = nhwc_ref(ref)
    t = Tally("fp32-patch dgrad tail", k)
    dyd, am, wdev = dev(L.nhwc(case.dy)), amax_r.to(DEV), dev(case.w)
    n = B * H * W * Ci
    whole = torch.full((GUARD + n + GUARD,), NAN, dtype=torch.float32, device=DEV)
    out = whole[GUARD:GUARD + n].view(B, H, W, Ci)
    got = ops.pconvf_dgrad(dyd, am, ops.pconvf_pack_weights(wdev), (B, H, W, Ci), out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == whole.data_ptr() + 4 * GUARD
    front, back = whole[:GUARD], whole[GUARD + n:]
    assert bool(torch.isnan(front).all()), f"{int((~torch.isnan(front)).sum())} stores in front of the tensor"
    assert bool(torch.isnan(back).all()), f"{int((~torch.isnan(back)).sum())} stores past the end of the tensor"
    t.eq("dX", got, dx_r)
    _, wd = ops.conv_pack_weights(wdev, Ci)
    t.eq("dX against the implicit-GEMM kernel's", got, ops.conv_dgrad(dyd, am, wd, (B, H, W, Ci), 1).cpu())
    t.done()


@pytest.mark.parametrize("shape,ni,segs", TAIL_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_last_tile(ops, shape, ni, segs):
    _, H, W, Ci, _ = shape
    assert tile_plan(H, W, Ci) == (segs, ni)
    run_case(ops, shape)


def stream_nis(B, H, W, Ci):
    """NI of every tile of every stream, in the order the stream's workgroup walks them"""
    segs, ni_last = tile_plan(H, W, Ci)
    return [[ni_last if u % segs == segs - 1 else 4 for u in range(s, B * segs, STREAMS)] for s in range(STREAMS)]


@pytest.mark.parametrize("shape,ni,segs", MIXED_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_a_stream_walks_tiles_of_mixed_row_block_counts(ops, shape, ni, segs):
    B, H, W, Ci, _ = shape
    assert tile_plan(H, W, Ci) == (segs, ni) and ni < 4 and Ci // (128 if Ci % 128 == 0 else 64) == 1
    walks = stream_nis(B, H, W, Ci)
    pairs = {(a, b) for w in walks for a, b in zip(w, w[1:])}
    assert (4, ni) in pairs and (ni, 4) in pairs and (4, 4) in pairs, pairs
    if B * segs > 2 * STREAMS:
        assert [4, ni, 4] in [w[:3] for w in walks]
    run_case(ops, shape)


@pytest.mark.parametrize("W", SWEEP_WIDTHS)
def test_epilogue_coordinates_over_widths(ops, W):
    run_case(ops, (1, 6, W, 64, 8))
