"""CPU: image preprocessing (vqa_preprocess_images, dl_vqa_amd.preprocess_images) -- the integer restatement against the
PIL-made fixtures and against PIL itself, the host-side coefficient / descriptor builders against the restatement, the crop's
banker's rounding, every argument error of the public call, and the ABI's host checks without a GPU."""
import re

import numpy as np
import pytest
import torch

from tests import preprocess_ref as R


@pytest.mark.parametrize("name", list(R.CASES))
def test_restatement_equals_fixture(name):
    g = R.golden()
    H, W, S, (num, den), seed = R.CASES[name]
    assert g["params/" + name].tolist() == [H, W, S, num, den, seed]          # the fixture was made for these parameters
    S, cf = R.case_args(name)
    got = R.preprocess(R.case_image(name), S, cf)
    assert got.dtype == torch.float16 and torch.equal(got, g[name])


def test_restatement_equals_fixture_before_the_fp16_rounding():
    S, cf = R.case_args(R.F32_CASE)
    got = R.preprocess(R.case_image(R.F32_CASE), S, cf, torch.float32)
    assert got.dtype == torch.float32 and torch.equal(got, R.golden()[R.F32_CASE + "/f32"])


@pytest.mark.parametrize("name", list(R.CASES))
def test_restatement_equals_pil(name):
    Image = pytest.importorskip("PIL.Image")
    H, W, S, (num, den), _ = R.CASES[name]
    cf = num / den
    img = R.case_image(name)
    oh, ow = R.resized_size(H, W, S, cf)
    top, left = R.crop_origin(oh, ow, S)
    pil = Image.fromarray(img, "RGB").resize((ow, oh), Image.BILINEAR).crop((left, top, left + S, top + S))
    assert np.array_equal(np.asarray(pil), R.preprocess_bytes(img, S, cf))


def test_issue_cases_exercise_what_they_name():
    """The geometry each case was chosen for, from the restatement's own rules."""
    def geo(name):
        H, W, S, (num, den), _ = R.CASES[name]
        oh, ow = R.resized_size(H, W, S, num / den)
        return H, W, S, oh, ow, R.crop_origin(oh, ow, S)
    assert geo("down_37x53")[3:5] == (16, 22) and geo("down_53x37")[3:5] == (22, 16)      # the short side either way
    H, W, S, oh, ow, _ = geo("up_20x20")
    # fs = 1: PIL's ksize is ceil(support) * 2 + 1 = 3 taps, of which the window [center - 1, center + 1) reaches 2 pixels
    assert (oh, ow) == (32, 32) and max(len(k) for _, k in R.coefficients(20, 32)) == 2
    assert geo("same_64x64")[3:5] == (64, 64)                                              # both passes skipped
    assert geo("vert_100x64")[3:5] == (100, 64)                                            # only the vertical pass
    assert geo("horiz_16x40")[3:5] == (16, 40)                                             # only the horizontal pass
    H, W, S, oh, ow, (top, left) = geo("frac_33x100")
    assert 0 < top < oh - S and 0 < left < ow - S                                          # strictly inside
    assert max(len(k) for _, k in R.coefficients(480, 32)) == 30                           # scale 15: ksize 31, 30 pixels reached
    assert all(18 % b for b in (4, 8, 16))                                                 # S = 18: no band divides it
    assert geo("down_100x64")[5][0] == 4 and geo("round_38x32")[5][0] == 2                 # 4.5 -> 4, 1.5 -> 2


# ---------------------------------------------------------------- the library's host side (no GPU)
def test_coefficient_builder_matches_the_restatement():
    from dl_vqa_amd import preprocess as P
    for n, m in [(53, 22), (37, 16), (20, 32), (100, 25), (480, 32), (640, 42), (33, 24), (100, 72), (7, 50), (1, 3), (3, 1)]:
        lo, ln, k = P.resample_coefficients(n, m)
        co = R.coefficients(n, m)
        assert lo.dtype == ln.dtype == k.dtype == np.int32 and k.shape == (m, int(ln.max()))
        for i, (l, kk) in enumerate(co):
            assert lo[i] == l and ln[i] == len(kk) and k[i, :len(kk)].tolist() == kk and not k[i, len(kk):].any()
        assert (lo >= 0).all() and (ln >= 1).all() and (lo + ln <= n).all()
        assert (np.abs(k.astype(np.int64).sum(1) - (1 << 22)) <= ln).all()                 # each row sums to 2^22 within len
    lo, ln, k = P.resample_coefficients(64, 64)                                            # the skipped pass: the identity
    assert lo.tolist() == list(range(64)) and (ln == 1).all() and (k == 1 << 22).all()


def _tables(P, desc, coef, S):
    for d in desc:
        for off, taps, n in ((d["h_off"], d["h_taps"], d["W"]), (d["v_off"], d["v_taps"], d["H"])):
            lo, ln = coef[off:off + S], coef[off + S:off + 2 * S]
            k = coef[off + 2 * S:off + 2 * S + S * taps].reshape(S, taps)
            yield d, n, lo, ln, k


def test_descriptor_builder_bounds_and_sums():
    from dl_vqa_amd import preprocess as P
    for names in (list(R.CASES)[:2], R.BATCH5, ["frac_33x100"], ["big_480x640", "up_20x20"], ["same_64x64", "vert_100x64"],
                  ["odd_41x29"]):
        S, cf = R.case_args(names[0])
        shapes = [R.CASES[n][:2] for n in names]
        desc, coef, src_bytes = P.build_plan(shapes, S, cf)
        assert desc.dtype.itemsize == 56 and coef.dtype == np.int32 and len(desc) == len(names)
        for d, n, lo, ln, k in _tables(P, desc, coef, S):
            assert (lo >= 0).all() and (ln >= 1).all() and (lo + ln <= n).all()            # every lo + len <= n
            assert (np.abs(k.astype(np.int64).sum(1) - (1 << 22)) <= ln).all()
        end = 0
        for d, (H, W) in zip(desc, shapes):
            oh, ow = R.resized_size(H, W, S, cf)
            assert (d["H"], d["W"], d["oh"], d["ow"]) == (H, W, oh, ow) and (d["top"], d["left"]) == R.crop_origin(oh, ow, S)
            assert d["pitch"] == 3 * W and d["src_offset"] >= end and d["src_offset"] % 16 == 0
            end = d["src_offset"] + H * W * 3
        assert src_bytes >= end
    # the window's table is the window of the axis table
    desc, coef, _ = P.build_plan([(33, 100)], 16, 16 / 24)
    d = desc[0]
    lo, ln, k = P.resample_coefficients(100, 72)
    assert coef[d["h_off"]:d["h_off"] + 16].tolist() == lo[d["left"]:d["left"] + 16].tolist()
    # images of one shape share their tables
    desc, coef, _ = P.build_plan([(37, 53)] * 3, 16, 1.0)
    assert len(set(desc["h_off"].tolist())) == 1 and len(set(desc["v_off"].tolist())) == 1


def test_host_plan_reproduces_the_fixtures():
    """The tables and the 3 x 256 look-up tables the kernel is given, applied by a few lines of numpy: equal to the fixtures."""
    from dl_vqa_amd import preprocess as P
    g = R.golden()
    for name in R.CASES:
        S, cf = R.case_args(name)
        img = R.case_image(name).astype(np.int64)
        desc, coef, _ = P.build_plan([img.shape[:2]], S, cf)
        (d, _, hlo, hln, hk), (_, _, vlo, vln, vk) = list(_tables(P, desc, coef, S))
        tmp = np.empty((img.shape[0], S, 3), dtype=np.int64)
        for x in range(S):
            acc = (img[:, hlo[x]:hlo[x] + hln[x], :] * hk[x, :hln[x]].astype(np.int64)[None, :, None]).sum(1)
            tmp[:, x, :] = np.clip((acc + (1 << 21)) >> 22, 0, 255)
        win = np.empty((S, S, 3), dtype=np.int64)
        for y in range(S):
            acc = (tmp[vlo[y]:vlo[y] + vln[y]] * vk[y, :vln[y]].astype(np.int64)[:, None, None]).sum(0)
            win[y] = np.clip((acc + (1 << 21)) >> 22, 0, 255)
        lut = P.normalize_table(torch.float16)
        got = torch.stack([lut[c][torch.from_numpy(win[:, :, c])] for c in range(3)])
        assert torch.equal(got, g[name]), name
    lut32 = P.normalize_table(torch.float32)
    assert lut32.dtype == torch.float32 and torch.equal(lut32.half(), P.normalize_table(torch.float16))
    b = torch.arange(256, dtype=torch.uint8).view(16, 16, 1).repeat(1, 1, 3).numpy()
    assert torch.equal(R.float_tail(b, torch.float32), torch.stack([lut32[c].view(16, 16) for c in range(3)]))


def test_crop_offsets_round_halves_to_even():
    from dl_vqa_amd import preprocess as P
    assert P.crop_origin(16, 17, 16) == (0, 0)            # (ow - S) = 1: 0.5 -> 0
    assert P.crop_origin(16, 19, 16) == (0, 2)            # (ow - S) = 3: 1.5 -> 2
    assert P.crop_origin(17, 16, 16) == (0, 0) and P.crop_origin(19, 16, 16) == (2, 0)
    assert P.crop_origin(21, 23, 16) == (2, 4)            # 2.5 -> 2, 3.5 -> 4
    assert P.crop_origin(24, 72, 16) == (4, 28)
    desc, _, _ = P.build_plan([(16, 17), (16, 19), (38, 32), (100, 64)], 16, 1.0)
    assert desc["left"].tolist() == [0, 2, 0, 0] and desc["top"].tolist() == [0, 0, 2, 4]
    assert P.resized_size(480, 640, 224) == (224, 298) and P.resized_size(640, 480, 224) == (298, 224)
    assert P.resize_target(16, 16 / 24) == 24 and P.resize_target(224, 0.875) == 256


# ---------------------------------------------------------------- argument errors of the public call, tensors on the CPU
def _img(H=20, W=24):
    return torch.zeros(H, W, 3, dtype=torch.uint8)


def test_public_name_and_signature():
    import inspect
    import dl_vqa_amd
    assert "preprocess_images" in dl_vqa_amd.__all__
    sig = inspect.signature(dl_vqa_amd.preprocess_images)
    assert list(sig.parameters) == ["images", "image_size", "central_fraction", "out_dtype", "device"]
    assert sig.parameters["central_fraction"].default == 1.0 and sig.parameters["out_dtype"].default == torch.float16
    assert sig.parameters["device"].default is None


def test_value_errors_come_before_any_device_work():
    from dl_vqa_amd import preprocess_images
    with pytest.raises(ValueError, match="uint8"):
        preprocess_images([_img().float()], 16)
    with pytest.raises(ValueError, match="uint8"):
        preprocess_images([np.zeros((20, 24, 3), dtype=np.int16)], 16)
    for bad in (torch.zeros(20, 24, dtype=torch.uint8), torch.zeros(20, 24, 4, dtype=torch.uint8),
                torch.zeros(3, 20, 24, dtype=torch.uint8), torch.zeros(1, 20, 24, 3, dtype=torch.uint8)):
        with pytest.raises(ValueError, match=r"\[H, W, 3\]"):
            preprocess_images([bad], 16)
    with pytest.raises(ValueError, match=r"\[N, H, W, 3\]"):
        preprocess_images(torch.zeros(20, 24, 3, dtype=torch.uint8), 16)          # a single image must come in a list
    for cf in (0.0, -0.5, 1.5, float("nan")):
        with pytest.raises(ValueError, match="central_fraction"):
            preprocess_images([_img()], 16, central_fraction=cf)
    with pytest.raises(ValueError, match="image_size"):
        preprocess_images([_img()], 0)
    with pytest.raises(ValueError, match="out_dtype"):
        preprocess_images([_img()], 16, out_dtype=torch.bfloat16)


def test_resized_side_below_image_size_is_refused():
    """With central_fraction in (0, 1] the short side resizes to int(S / cf) >= S, so the public call cannot get there; the
    guard sits in the plan builder (and in the ABI, test_argument_validation_without_gpu) for callers that build plans."""
    from dl_vqa_amd import preprocess as P
    with pytest.raises(ValueError, match="smaller than image_size"):
        P.build_plan([(20, 24)], 16, central_fraction=2.0)                         # R = 8: 8 x 9
    with pytest.raises(ValueError, match="smaller than image_size"):
        P.build_plan([(64, 64), (20, 24)], 16, central_fraction=1.25)              # R = 12


def test_runtime_error_without_a_cuda_device():
    from dl_vqa_amd import preprocess_images
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        preprocess_images([_img()], 16)                                            # host images, no device named
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        preprocess_images([_img()], 16, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        preprocess_images([], 16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        preprocess_images(np.zeros((2, 20, 24, 3), dtype=np.uint8), 16)


def test_uncovered_scale_is_a_value_error():
    """One output row of S = 1024 from a 10240 x 10240 image reads 20 source rows of 3072 bytes: more than the LDS tile.
    (The image is a stride-0 view: the error comes before a pixel is read.)"""
    from dl_vqa_amd import ops, preprocess as P, preprocess_images
    desc, coef, _ = P.build_plan([(10240, 10240)], 1024, 1.0)
    assert ops.preprocess_supported(desc, coef, 1024) == 0 and "not covered" in ops.last_error()
    with pytest.raises(ValueError, match="not covered"):
        preprocess_images([torch.zeros(1, 1, 3, dtype=torch.uint8).expand(10240, 10240, 3)], 1024)
    desc, coef, _ = P.build_plan([(480, 640)], 32, 1.0)                      # scale 15 is covered, with the full band
    assert ops.preprocess_supported(desc, coef, 32) == 16


# ---------------------------------------------------------------- the ABI without a GPU
def test_entry_points_in_header_prototypes_and_library():
    from dl_vqa_amd import _lib, build
    build.build_library(verbose=False)
    with open(_lib.HEADER_PATH) as f:
        header = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    lib = _lib.load()
    for name in ("vqa_preprocess_images", "vqa_preprocess_supported"):
        assert re.search(r"\b%s\s*\(" % name, header) and name in _lib.PROTOTYPES and hasattr(lib, name)
    assert lib.vqa_abi_version() == _lib.header_abi_version() == 9              # 9 since vqa_conv3x3_x3_plan
    from dl_vqa_amd import preprocess as P
    m = re.search(r"typedef struct \{([^{}]*)\} vqa_pre_image_t;", header)
    fields = re.findall(r"\b(\w+)\s*[,;]", m.group(1))
    assert fields == list(P.DESC_DTYPE.names)                                    # the numpy record is the C struct


def test_argument_validation_without_gpu():
    """Every check runs on the host before any HIP call.  Arguments: src, src_bytes, images_host, coef_host, coef_len,
    images_dev, coef_dev, N, S, lut, out_is_f32, out, stream (device pointers are made-up integers: nothing reads them)."""
    from dl_vqa_amd import _lib, ops, preprocess as P
    lib = _lib.load()
    f = lib.vqa_preprocess_images
    desc, coef, nbytes = P.build_plan([(37, 53), (53, 37)], 16, 1.0)
    dp, cp, n = desc.ctypes.data, coef.ctypes.data, coef.size

    def err(rc, text):
        return rc == 1 and text in lib.vqa_last_error()
    assert ops.preprocess_supported(desc, coef, 16) == 16                         # the band height
    assert err(f(16, nbytes, dp, cp, n, 16, 16, -1, 16, 16, 0, 16, None), b"N=-1")
    assert err(f(16, nbytes, dp, cp, n, 16, 16, 2, 0, 16, 0, 16, None), b"S=0")
    assert f(None, 0, None, None, 0, None, None, 0, 16, None, 0, None, None) == 0     # N = 0: OK, nothing is read
    assert err(f(None, 0, None, None, 0, None, None, 0, 0, None, 0, None, None), b"S=0")   # ... but S is checked
    assert err(f(16, nbytes, None, cp, n, 16, 16, 2, 16, 16, 0, 16, None), b"null pointer")     # images_host
    assert err(f(16, nbytes, dp, None, n, 16, 16, 2, 16, 16, 0, 16, None), b"null pointer")     # coef_host
    for k in (0, 5, 6, 9, 11):                                                                    # src, *_dev, lut, out
        args = [16, nbytes, dp, cp, n, 16, 16, 2, 16, 16, 0, 16, None]
        args[k] = None
        assert err(f(*args), b"null pointer"), k
    end = int(desc["src_offset"][1]) + 53 * 37 * 3
    assert err(f(16, end - 1, dp, cp, n, 16, 16, 2, 16, 16, 0, 16, None), b"outside the")           # the last image's bytes
    bad = desc.copy()
    bad["pitch"][0] = 3 * 53 - 1
    assert err(f(16, nbytes, bad.ctypes.data, cp, n, 16, 16, 2, 16, 16, 0, 16, None), b"pitch")
    bad = desc.copy()
    bad["oh"][1] = 15                                                                               # a resized side below S
    assert err(f(16, nbytes, bad.ctypes.data, cp, n, 16, 16, 2, 16, 16, 0, 16, None), b"smaller than S")
    bad = desc.copy()
    bad["left"][0] = 7                                                                              # ow - S = 6
    assert err(f(16, nbytes, bad.ctypes.data, cp, n, 16, 16, 2, 16, 16, 0, 16, None), b"crop origin")
    bad = desc.copy()
    bad["v_off"][1] = n - 8
    assert err(f(16, nbytes, bad.ctypes.data, cp, n, 16, 16, 2, 16, 16, 0, 16, None), b"outside coef")
    badc = coef.copy()
    badc[desc["h_off"][0] + 15] = 53                                                                # lo + len > W
    assert err(f(16, nbytes, dp, badc.ctypes.data, n, 16, 16, 2, 16, 16, 0, 16, None), b"table entry 15")
    badc = coef.copy()
    badc[desc["v_off"][0] + 16] = 0                                                                 # len = 0
    assert err(f(16, nbytes, dp, badc.ctypes.data, n, 16, 16, 2, 16, 16, 0, 16, None), b"table entry 0")
    assert lib.vqa_preprocess_supported(dp, badc.ctypes.data, n, 2, 16) == 0
