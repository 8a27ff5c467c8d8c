"""CPU: vqa_conv3x3_x3_plan (ops.conv_x3_plan) -- the tile, the tile counts, the persistent rule, the batch chunk and the
wgrad split plan that the fp32x3 conv launchers of csrc/conv_x3.hip decide, from the host functions those launchers call.  No
HIP call is made, so every check here runs without a GPU.  The expectations are worked out by hand from the rules as
include/vqa_hip.h and csrc/conv_x3.hip state them (192 x 128 tiles for more than 64 output columns, else 256 x 64, the dgrad
one with 16 waves; persistent above 256 tiles; wgrad: 192 x 128 tiles on 256 slots, at least 8 K-steps of 32 pixels a split),
for the shapes tests/test_conv_lattice_gpu.py asserts its variants with."""
import ctypes
import os

import pytest

from tests import conv_lattice_ref as L


@pytest.fixture()
def ops(monkeypatch):
    """dl_vqa_amd.ops with no VQA_* knob in force (the knobs are read once per process, other tests may have set some)"""
    from dl_vqa_amd import _lib, ops
    for k in [k for k in os.environ if k.startswith("VQA_") and k != "VQA_LIB"]:
        monkeypatch.delenv(k)
    _lib.load().vqa_reload_knobs()
    yield ops
    monkeypatch.undo()
    _lib.load().vqa_reload_knobs()


def _ceil(a, b):
    return -(-a // b)


# (B, H, W, CiP, Co, stride) -> forward (BM, BN, waves, tiles_m, tiles_n, persistent), dgrad (the same)
TILES = {
    (2, 36, 36, 32, 64, 1): ((256, 64, 8, 10, 1, 0), (256, 64, 16, 11, 1, 0)),         # 2312 conv pixels, 2592 input pixels
    (1, 36, 36, 96, 128, 1): ((192, 128, 8, 7, 1, 0), (192, 128, 8, 7, 1, 0)),         # 1156 and 1296
    (2, 37, 67, 32, 64, 2): ((256, 64, 8, 5, 1, 0), (256, 64, 16, 20, 1, 0)),          # Hp = 9, Wp = 16: 1152 and 4958
    (4, 114, 114, 96, 128, 1): ((192, 128, 8, 262, 1, 1), (192, 128, 8, 271, 1, 1)),   # 50176 and 51984
    (6, 114, 114, 64, 64, 1): ((256, 64, 8, 294, 1, 1), (256, 64, 16, 305, 1, 1)),     # 75264 and 77976
    (2, 36, 36, 64, 128, 1): ((192, 128, 8, 13, 1, 0), (256, 64, 16, 11, 1, 0)),       # a wide forward over a narrow dgrad
    (2, 36, 36, 160, 160, 1): ((192, 128, 8, 13, 2, 0), (192, 128, 8, 14, 2, 0)),      # two column tiles
}
FIELDS = ("BM", "BN", "waves", "tiles_m", "tiles_n", "persistent")


def test_the_gpu_file_asserts_its_variants_on_shapes_of_this_table():
    assert set(L.PLANE_SHAPES + [L.PLANE_STRIDE2] + L.X3_PERSISTENT_CASES) <= set(TILES)


@pytest.mark.parametrize("shape", TILES, ids=str)
def test_forward_and_dgrad_tiles(ops, shape):
    B, H, W, CiP, Co, stride = shape
    for pass_, want in zip(("forward", "dgrad"), TILES[shape]):
        plan = ops.conv_x3_plan(pass_, B, H, W, CiP, Co, stride)
        assert tuple(plan[f] for f in FIELDS) == want, (pass_, plan)
        nk = 9 * (CiP if pass_ == "forward" else Co) // 32
        assert (plan["chunk"], plan["launches"], plan["nk"], plan["splits"], plan["ks_per_split"]) == (B, 1, nk, 1, nk)
        assert plan["tiles"] == want[3] * want[4] and (plan["tiles"] > 256) == bool(want[5])


@pytest.mark.parametrize("shape", TILES, ids=str)
def test_wgrad_split_plan(ops, shape):
    """192 x 128 tiles of dW [9 CiP][Co], K-steps of 32 over the B * 2Hp * 2Wp pool-covered conv pixels, as many splits as
    256 slots hold but at least 8 K-steps each"""
    B, H, W, CiP, Co, stride = shape
    _, _, Hp, Wp = L.out_hw(H, W, 3, stride)
    plan = ops.conv_x3_plan("wgrad", B, H, W, CiP, Co, stride)
    tiles_m, tiles_n, nk = _ceil(9 * CiP, 192), _ceil(Co, 128), _ceil(B * 4 * Hp * Wp, 32)
    splits = min(max(256 // (tiles_m * tiles_n), 1), max(nk // 8, 1))
    ks = _ceil(nk, splits)
    assert (plan["BM"], plan["BN"], plan["waves"], plan["persistent"]) == (192, 128, 8, 0)
    assert (plan["tiles_m"], plan["tiles_n"], plan["nk"], plan["ks_per_split"], plan["splits"]) == (tiles_m, tiles_n, nk, ks, _ceil(nk, ks))
    assert ks >= 8 or plan["splits"] == 1


def test_wgrad_split_plan_by_hand(ops):
    plan = ops.conv_x3_plan("wgrad", 2, 36, 36, 32, 64, 1)           # 288 x 64: 2 x 1 tiles; 2312 pixels: 73 K-steps, 9 splits of 9
    assert (plan["tiles_m"], plan["tiles_n"], plan["nk"], plan["splits"], plan["ks_per_split"]) == (2, 1, 73, 9, 9)
    plan = ops.conv_x3_plan("wgrad", 4, 114, 114, 96, 128, 1)        # 864 x 128: 5 x 1 tiles, 51 slots each; 1568 K-steps of 31
    assert (plan["tiles_m"], plan["tiles_n"], plan["nk"], plan["splits"], plan["ks_per_split"]) == (5, 1, 1568, 51, 31)


def test_the_knobs_in_force_decide(ops, monkeypatch):
    from dl_vqa_amd import _lib
    shape = (4, 114, 114, 96, 128, 1)
    monkeypatch.setenv("VQA_PERSISTENT", "0")
    _lib.load().vqa_reload_knobs()
    for pass_, want in zip(("forward", "dgrad"), TILES[shape]):
        plan = ops.conv_x3_plan(pass_, *shape)
        assert tuple(plan[f] for f in FIELDS) == want[:5] + (0,), plan
    monkeypatch.delenv("VQA_PERSISTENT")
    monkeypatch.setenv("VQA_CONV_CHUNK", "2")
    _lib.load().vqa_reload_knobs()
    B, H, W, CiP, Co, stride = L.X3_CHUNK_CASE
    assert B == 5
    for pass_ in ("forward", "dgrad", "wgrad"):
        plan = ops.conv_x3_plan(pass_, B, H, W, CiP, Co, stride)
        two = ops.conv_x3_plan(pass_, 2, H, W, CiP, Co, stride)                   # the first launch: two images
        assert (plan["chunk"], plan["launches"]) == (2, 3) and (two["chunk"], two["launches"]) == (2, 1)
        assert {f: plan[f] for f in plan if f != "launches"} == {f: two[f] for f in two if f != "launches"}
    assert ops.conv_x3_plan("forward", B, H, W, CiP, Co, stride)["tiles_m"] == _ceil(2 * 4 * 18 * 20, 192)


def test_bad_arguments_return_the_librarys_error(ops):
    from dl_vqa_amd import _lib
    lib = _lib.load()
    out = (ctypes.c_int32 * 11)()
    good = (0, 2, 36, 36, 32, 64, 1)
    assert lib.vqa_conv3x3_x3_plan(*good, out, 11) == 0 and out[0] == 256
    bad = {
        "pass 3": ((3,) + good[1:], out, 11),
        "pass -1": ((-1,) + good[1:], out, 11),
        "B = 0": ((0, 0) + good[2:], out, 11),
        "short out": (good, out, 10),
        "null out": (good, None, 11),
        "image too small": ((0, 2, 3, 36, 32, 64, 1), out, 11),
        "stride 3": ((0, 2, 36, 36, 32, 64, 3), out, 11),
        "stride 0": ((0, 2, 36, 36, 32, 64, 0), out, 11),
        "CiP = 48": ((0, 2, 36, 36, 48, 64, 1), out, 11),
        "Co = 40": ((0, 2, 36, 36, 32, 40, 1), out, 11),
        "a conv row under 32 pixels": ((0, 2) + L.X3_NOT_ADMITTED, out, 11),
    }
    for what, (args, o, n) in bad.items():
        rc = lib.vqa_conv3x3_x3_plan(*args, o, n)
        assert rc == 1 and lib.vqa_last_error().startswith(b"vqa_conv3x3_x3_plan:"), (what, rc, lib.vqa_last_error())
    with pytest.raises(_lib.VqaHipError, match="vqa_conv3x3_x3_plan: bad args"):
        ops.conv_x3_plan("forward", 0, 36, 36, 32, 64, 1)
    with pytest.raises(KeyError):
        ops.conv_x3_plan("backward", 2, 36, 36, 32, 64, 1)
    for shape in TILES:                                    # every layer the query answers is one the entry points admit
        assert ops.conv_x3_supported(*shape[1:])
