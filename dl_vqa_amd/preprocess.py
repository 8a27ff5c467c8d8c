"""Raw RGB images -> the model's input tensor on the device, bit for bit what the reference's host pipeline computes
(preprocessing/preprocess_images.py:8-15,50-52: Resize(int(S / cf)), CenterCrop(S), ToTensor, Normalize, .astype('float16')).

The semantics are stated once in include/vqa_hip.h ("image preprocessing") and DESIGN.md 4.11.  This module holds the host
side, which needs no GPU: the resize / crop geometry (`resized_size`, `crop_origin`), PIL's bilinear coefficient tables in
22-bit fixed point (`resample_coefficients`, cached per (n, m)), the 3 x 256 look-up tables of the float tail
(`normalize_table`), and `build_plan`, which lays descriptors and coefficient tables out the way csrc/preprocess.hip reads
them.  `preprocess_images` is the public call: it packs host images into one pinned staging buffer, uploads once and
launches one kernel for the whole batch."""
from __future__ import annotations

import functools
from typing import List, Sequence, Tuple

import numpy as np
import torch

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
PRECISION_BITS = 22                      # PIL's 8-bit resample: coefficients are int(0.5 + w * 2^22)

# vqa_pre_image_t (include/vqa_hip.h), 56 bytes
DESC_DTYPE = np.dtype([("src_offset", "<i8"), ("pitch", "<i8"), ("H", "<i4"), ("W", "<i4"), ("oh", "<i4"), ("ow", "<i4"),
                       ("top", "<i4"), ("left", "<i4"), ("h_off", "<i4"), ("h_taps", "<i4"), ("v_off", "<i4"),
                       ("v_taps", "<i4")])
assert DESC_DTYPE.itemsize == 56


def resize_target(image_size: int, central_fraction: float) -> int:
    """Step 1: the length the short side is resized to (preprocess_images.py:10)."""
    return int(image_size / central_fraction)


def resized_size(H: int, W: int, R: int) -> Tuple[int, int]:
    """(oh, ow) of Resize(R) on an H x W image: the short side becomes R, the long side int(R * long / short)."""
    if W <= H:
        return int(R * H / W), R
    return R, int(R * W / H)


def crop_origin(oh: int, ow: int, S: int) -> Tuple[int, int]:
    """(top, left) of CenterCrop(S) in an oh x ow image.  Python's round: halves go to the even integer."""
    return int(round((oh - S) / 2.0)), int(round((ow - S) / 2.0))


@functools.lru_cache(maxsize=256)
def resample_coefficients(n: int, m: int):
    """PIL's antialiased bilinear resample of an axis from n to m samples (Resample.c precompute_coeffs +
    normalize_coeffs_8bpc), computed in double in PIL's operation order.  Returns (lo [m], len [m], k [m, taps]) int32:
    output i = clip((2^21 + sum_x in[lo[i] + x] * k[i, x]) >> 22, 0, 255), x < len[i]; k is 0 past len[i].
    n == m is the skipped pass: one tap of exactly 2^22, which reproduces the byte."""
    if n == m:
        return (np.arange(m, dtype=np.int32), np.ones(m, dtype=np.int32),
                np.full((m, 1), 1 << PRECISION_BITS, dtype=np.int32))
    scale = n / m
    fs = max(scale, 1.0)
    support = 1.0 * fs                                  # the bilinear filter's support is 1
    ss = 1.0 / fs
    center = (np.arange(m, dtype=np.float64) + 0.5) * scale
    lo = np.maximum((center - support + 0.5).astype(np.int64), 0)       # (int): truncation
    hi = np.minimum((center + support + 0.5).astype(np.int64), n)
    ln = hi - lo
    taps = int(ln.max())
    x = np.arange(taps, dtype=np.int64)[None, :]
    arg = ((x + lo[:, None]) - center[:, None] + 0.5) * ss
    w = np.where(x < ln[:, None], np.maximum(0.0, 1.0 - np.abs(arg)), 0.0)
    ww = np.zeros(m, dtype=np.float64)
    for j in range(taps):                               # the sum runs in tap order, as the C loop does
        ww = ww + w[:, j]
    w = np.where(ww[:, None] != 0.0, w / np.where(ww == 0.0, 1.0, ww)[:, None], w)
    k = (0.5 + w * float(1 << PRECISION_BITS)).astype(np.int64)         # every bilinear weight is >= 0
    out = (lo.astype(np.int32), ln.astype(np.int32), k.astype(np.int32))
    for a in out:                                       # cached: shared between callers
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=256)
def _window_table(n: int, m: int, start: int, S: int) -> np.ndarray:
    """The flat int32 table the kernel reads for output samples start .. start + S of an n -> m axis:
    lo[S], len[S], k[S][taps]."""
    lo, ln, k = resample_coefficients(n, m)
    t = np.concatenate([lo[start:start + S], ln[start:start + S], k[start:start + S].reshape(-1)]).astype(np.int32)
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=4)
def normalize_table(dtype=torch.float16) -> torch.Tensor:
    """Step 4 as a [3, 256] CPU table: ToTensor (byte -> fp32, / 255), Normalize ((x - mean) / std in fp32), then the
    dataset's fp16 rounding unless dtype is float32.  Built with torch CPU ops in the reference's operation order, so a
    look-up is exact by construction."""
    x = torch.arange(256, dtype=torch.uint8).to(torch.float32).div(255)
    x = x[None, :].repeat(3, 1)
    x.sub_(torch.tensor(MEAN, dtype=torch.float32)[:, None]).div_(torch.tensor(STD, dtype=torch.float32)[:, None])
    return x.half() if dtype == torch.float16 else x


def build_plan(shapes: Sequence[Tuple[int, int]], image_size: int, central_fraction: float = 1.0, offsets=None, pitches=None):
    """Descriptors and coefficient tables for a batch of images of the given (H, W).  Returns (desc, coef, src_bytes):
    desc a DESC_DTYPE array [N], coef one int32 array holding every distinct table once, src_bytes the size of the packed
    source buffer (images back to back, each starting at a multiple of 16 bytes, unless offsets / pitches are given).
    ValueError where a resized side falls below image_size."""
    S = int(image_size)
    R = resize_target(S, central_fraction)
    desc = np.zeros(len(shapes), dtype=DESC_DTYPE)
    tables: List[np.ndarray] = []
    where = {}
    used = 0
    pos = 0

    def table(n, m, start):
        nonlocal used
        key = (n, m, start)
        if key not in where:
            t = _window_table(n, m, start, S)
            where[key] = (used, (len(t) - 2 * S) // S)
            tables.append(t)
            used += len(t)
        return where[key]

    for i, (H, W) in enumerate(shapes):
        H, W = int(H), int(W)
        if H < 1 or W < 1:
            raise ValueError(f"preprocess_images: image {i} is empty ({H} x {W})")
        oh, ow = resized_size(H, W, R)
        if oh < S or ow < S:
            raise ValueError(f"preprocess_images: image {i} ({H} x {W}) resizes to {oh} x {ow}, smaller than image_size={S} "
                             "(the reference's CenterCrop would pad; this path refuses)")
        top, left = crop_origin(oh, ow, S)
        d = desc[i]
        d["H"], d["W"], d["oh"], d["ow"], d["top"], d["left"] = H, W, oh, ow, top, left
        d["h_off"], d["h_taps"] = table(W, ow, left)
        d["v_off"], d["v_taps"] = table(H, oh, top)
        d["pitch"] = 3 * W if pitches is None else int(pitches[i])
        if offsets is None:
            d["src_offset"] = pos
            pos += (H * W * 3 + 15) // 16 * 16
        else:
            d["src_offset"] = int(offsets[i])
            pos = max(pos, int(offsets[i]) + (H - 1) * int(d["pitch"]) + 3 * W)
    coef = np.concatenate(tables) if tables else np.zeros(0, dtype=np.int32)
    return desc, coef, pos


def model_bytes(desc: np.ndarray, coef: np.ndarray, image_size: int, out_itemsize: int = 2) -> int:
    """The byte model of the kernel: the source bytes of the rows and columns the crop window needs, once,
    plus the output planes (6 * S * S for fp16)."""
    S = int(image_size)
    total = 0
    for d in desc:
        h = coef[d["h_off"]: d["h_off"] + 2 * S]
        v = coef[d["v_off"]: d["v_off"] + 2 * S]
        cols = int((h[:S] + h[S:]).max() - h[:S].min())
        rows = int((v[:S] + v[S:]).max() - v[:S].min())
        total += rows * cols * 3 + 3 * S * S * out_itemsize
    return total


_staging = {}      # device -> (pinned uint8 tensor, event of the last upload that read it)
_luts = {}         # (device, dtype) -> device table


def _device_lut(device, dtype):
    key = (str(device), dtype)
    if key not in _luts:
        _luts[key] = normalize_table(dtype).to(device)
    return _luts[key]


def _staging_buffer(device, nbytes: int) -> torch.Tensor:
    """A pinned host buffer that only grows, one per device.  The previous call's upload is waited for before the
    buffer is written again."""
    buf, ev = _staging.get(str(device), (None, None))
    if ev is not None:
        ev.synchronize()
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, pin_memory=True)
    _staging[str(device)] = (buf, None)
    return buf


def _host_tensor(im) -> torch.Tensor:
    if isinstance(im, np.ndarray) and any(st < 0 for st in im.strides):
        im = np.ascontiguousarray(im)                   # torch takes no negative strides
    return torch.as_tensor(im)


def _as_image_list(images):
    if isinstance(images, (torch.Tensor, np.ndarray)):
        if images.ndim != 4:
            raise ValueError(f"preprocess_images: a list of [H, W, 3] images or one [N, H, W, 3] array expected, got shape "
                             f"{tuple(images.shape)}")
        return [images[i] for i in range(images.shape[0])], images
    return list(images), None


def preprocess_images(images, image_size: int, central_fraction: float = 1.0, out_dtype=torch.float16, device=None):
    """Resize, centre-crop and normalise raw RGB images on the device: what the reference's
    preprocessing/preprocess_images.py computes per image through PIL and torchvision, bit for bit, in one kernel launch.

    images: a list of uint8 [H, W, 3] torch tensors or numpy arrays (any mix of sizes, host or device, possibly
    non-contiguous), or one uint8 [N, H, W, 3] tensor / array.  The short side is resized to int(image_size /
    central_fraction) with PIL's antialiased bilinear filter, the centre image_size x image_size window is cut out
    (Python's round for the offsets), and every byte b of channel c becomes ((b / 255) - mean[c]) / std[c] in fp32,
    rounded to fp16 unless out_dtype is torch.float32.  Returns the CUDA tensor [N, 3, image_size, image_size] (NCHW, the
    dataset's storage format), which encode_images and forward read as it is.

    Host images are packed into one pinned staging buffer and uploaded once, on the current stream.  `device` names
    the target; without it the device of the first CUDA image is used.  ValueError (before any device work) for a dtype
    other than uint8, a shape other than [H, W, 3], central_fraction outside (0, 1], an out_dtype other than
    float16 / float32, or a resized side below image_size (CenterCrop would pad; this path refuses) and for a shape
    the kernel does not cover; RuntimeError when no CUDA device is given or implied (there is no CPU fallback).
    An empty list gives an empty [0, 3, S, S] tensor.  JPEG decoding and file handling stay with the caller."""
    from . import ops
    if isinstance(image_size, bool) or not isinstance(image_size, (int, np.integer)) or image_size < 1:
        raise ValueError(f"preprocess_images: image_size={image_size!r} must be an int >= 1")
    S = int(image_size)
    cf = float(central_fraction)
    if not (0.0 < cf <= 1.0):
        raise ValueError(f"preprocess_images: central_fraction={central_fraction!r} outside (0, 1]")
    if out_dtype not in (torch.float16, torch.float32):
        raise ValueError(f"preprocess_images: out_dtype={out_dtype} (torch.float16 or torch.float32)")
    imgs, whole = _as_image_list(images)
    for i, im in enumerate(imgs):
        if not isinstance(im, (torch.Tensor, np.ndarray)):
            raise ValueError(f"preprocess_images: image {i} is a {type(im).__name__}; torch tensors or numpy arrays expected")
        if im.dtype not in (torch.uint8, np.uint8):
            raise ValueError(f"preprocess_images: image {i} has dtype {im.dtype}; uint8 expected")
        if im.ndim != 3 or im.shape[2] != 3:
            raise ValueError(f"preprocess_images: image {i} has shape {tuple(im.shape)}; [H, W, 3] expected")
    shapes = [(int(im.shape[0]), int(im.shape[1])) for im in imgs]
    desc, coef, src_bytes = build_plan(shapes, S, cf)                 # ValueError: a resized side below S
    if imgs and ops.preprocess_supported(desc, coef, S) == 0:         # host-side query: no device needed
        raise ValueError("preprocess_images: " + ops.last_error())
    if device is None:
        device = next((im.device for im in imgs if isinstance(im, torch.Tensor) and im.is_cuda), None)
    if device is None or torch.device(device).type != "cuda":
        raise RuntimeError("dl_vqa_amd.preprocess_images needs a CUDA (HIP) device: pass device= or a CUDA image; "
                           "there is no CPU fallback")
    device = torch.device(device)
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    N = len(imgs)
    if N == 0:
        return torch.empty(0, 3, S, S, dtype=out_dtype, device=device)

    with torch.cuda.device(device):
        in_place = (isinstance(whole, torch.Tensor) and whole.device == device and whole.is_contiguous())
        if in_place:                        # one contiguous [N, H, W, 3] device tensor is read where it lies
            H, W = shapes[0]
            desc["src_offset"] = np.arange(N, dtype=np.int64) * (H * W * 3)
            src_bytes = N * H * W * 3
        on_host = [not (isinstance(im, torch.Tensor) and im.is_cuda) for im in imgs]
        if not in_place:                    # host images first: they travel with the plan in one upload
            pos = 0
            for want in (True, False):
                for i, (H, W) in enumerate(shapes):
                    if on_host[i] == want:
                        desc["src_offset"][i] = pos
                        pos += (H * W * 3 + 15) // 16 * 16
                if want:
                    host_bytes = pos
            src_bytes = pos
        else:
            host_bytes = 0
        desc_bytes = (desc.nbytes + 15) // 16 * 16
        plan_bytes = desc_bytes + (coef.nbytes + 15) // 16 * 16
        stage = _staging_buffer(device, plan_bytes + host_bytes)
        stage[:desc.nbytes].copy_(torch.from_numpy(desc.view(np.uint8)))
        stage[desc_bytes:desc_bytes + coef.nbytes].copy_(torch.from_numpy(coef.view(np.uint8)))
        if not in_place:
            for i, im in enumerate(imgs):
                if on_host[i]:
                    H, W = shapes[i]
                    o = plan_bytes + int(desc["src_offset"][i])
                    stage[o:o + H * W * 3].view(H, W, 3).copy_(_host_tensor(im))
        dbuf = torch.empty(plan_bytes + (0 if in_place else src_bytes), dtype=torch.uint8, device=device)
        dbuf[:plan_bytes + host_bytes].copy_(stage[:plan_bytes + host_bytes], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        _staging[str(device)] = (stage, ev)
        if not in_place:
            for i, im in enumerate(imgs):
                if not on_host[i]:
                    H, W = shapes[i]
                    o = plan_bytes + int(desc["src_offset"][i])
                    dbuf[o:o + H * W * 3].view(H, W, 3).copy_(im)      # device to device; any strides, any device
        src = whole.view(-1) if in_place else dbuf[plan_bytes:]
        out = torch.empty(N, 3, S, S, dtype=out_dtype, device=device)
        ops.preprocess_images(src, src_bytes, desc, coef, dbuf[:desc.nbytes], dbuf[desc_bytes:desc_bytes + coef.nbytes], S,
                              _device_lut(device, out_dtype), out)
    return out
