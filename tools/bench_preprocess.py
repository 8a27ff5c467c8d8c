"""Image preprocessing on the device: dl_vqa_amd.preprocess_images on 256 images of 480 x 640, to S = 224 and to S = 448
(central_fraction 1), against the reference's host pipeline and against torch's own resize on the device.

    python tools/bench_preprocess.py [--out-dir profiles] [--reps 7] [--iters 20] [--images 256]

Per case, all timed in this one process on the same machine:
  call_ms / images_per_s   the public call on HOST images (plan, packing into the pinned buffer, one upload, the kernel),
                           host clock around the call and a device synchronise, median over --reps
  device_call_ms           the same call on one device-resident [N, H, W, 3] tensor (read in place: no pixel upload)
  upload_share             1 - device_call_ms / call_ms: the share of the call spent packing and uploading pixels
  kernel_ms                the launch alone (ops.preprocess_images on a prepared plan), HIP events around --iters launches
  model_bytes              source bytes of the rows and columns the crop window needs + 6 * S * S per image
  kernel_bytes_per_s       model_bytes / kernel time, with its fraction of the 8 TB/s HBM3E peak
  pil_images_per_s         the reference chain through PIL on one host core (only where PIL is importable)
  torch_ms                 torch.nn.functional.interpolate(mode="bilinear", antialias=True) + crop + normalise + half on
                           the device, pixels already resident: a speed baseline only, it is not bit-identical
Output: one JSON line on stdout and OUT_DIR/preprocess_bench.json."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W = 480, 640
HBM_PEAK = 8.0e12


def _images(n):
    import numpy as np
    from tests.preprocess_ref import synthetic_image
    distinct = [synthetic_image(H, W, s) for s in range(8)]
    return np.stack([distinct[i % 8] for i in range(n)])


def _events(fn, iters):
    import torch
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters


def _wall(fn):
    import torch
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def _pil_rate(imgs, S, n=8):
    try:
        from PIL import Image
    except ImportError:
        return None
    import numpy as np
    import torch
    from dl_vqa_amd import preprocess as P
    torch.set_num_threads(1)
    mean = torch.tensor(P.MEAN)[:, None, None]
    std = torch.tensor(P.STD)[:, None, None]
    oh, ow = P.resized_size(H, W, S)
    top, left = P.crop_origin(oh, ow, S)
    t = time.perf_counter()
    for i in range(n):
        im = Image.fromarray(imgs[i], "RGB").resize((ow, oh), Image.BILINEAR).crop((left, top, left + S, top + S))
        x = torch.from_numpy(np.array(im)).permute(2, 0, 1).contiguous().to(torch.float32).div(255)
        x.sub_(mean).div_(std)
        x.numpy().astype("float16")
    return n / (time.perf_counter() - t)


def case(imgs, S, reps, iters):
    import torch
    import torch.nn.functional as F
    from dl_vqa_amd import ops, preprocess as P, preprocess_images
    N = len(imgs)
    host = torch.from_numpy(imgs)
    dev = host.cuda()
    med = statistics.median
    for _ in range(2):                                   # warm-up: code objects, the pinned buffer, the allocator
        preprocess_images(host, S, device="cuda")
        preprocess_images(dev, S)
    call = med(_wall(lambda: preprocess_images(host, S, device="cuda")) for _ in range(reps))
    dcall = med(_wall(lambda: preprocess_images(dev, S)) for _ in range(reps))

    desc, coef, _ = P.build_plan([(H, W)] * N, S, 1.0, offsets=[i * H * W * 3 for i in range(N)])
    desc_d = torch.from_numpy(desc.view("uint8")).cuda()
    coef_d = torch.from_numpy(coef.view("uint8")).cuda()
    lut = P.normalize_table(torch.float16).cuda()
    out = torch.empty(N, 3, S, S, dtype=torch.float16, device="cuda")
    src = dev.view(-1)

    def launch():
        ops.preprocess_images(src, src.numel(), desc, coef, desc_d, coef_d, S, lut, out)
    launch()
    kern = med(_events(launch, iters) for _ in range(reps))
    nbytes = P.model_bytes(desc, coef, S)

    oh, ow = P.resized_size(H, W, S)
    top, left = P.crop_origin(oh, ow, S)
    mean = torch.tensor(P.MEAN, device="cuda")[None, :, None, None]
    std = torch.tensor(P.STD, device="cuda")[None, :, None, None]

    def torch_path():
        x = dev.permute(0, 3, 1, 2).float()
        x = F.interpolate(x, size=(oh, ow), mode="bilinear", antialias=True, align_corners=False)
        x = x[:, :, top:top + S, left:left + S]
        return ((x / 255 - mean) / std).half()
    torch_path()
    tms = med(_events(torch_path, 3) for _ in range(reps))
    pil = _pil_rate(imgs, S)
    bps = nbytes / (kern * 1e-3)
    return {"S": S, "images": N, "source": [H, W], "band_rows": ops.preprocess_supported(desc, coef, S),
            "call_ms": round(call, 3), "images_per_s": round(N / (call * 1e-3)), "device_call_ms": round(dcall, 3),
            "upload_share": round(max(0.0, 1 - dcall / call), 3), "kernel_ms": round(kern, 4),
            "kernel_images_per_s": round(N / (kern * 1e-3)), "model_bytes": nbytes,
            "kernel_bytes_per_s": round(bps), "fraction_of_hbm_peak": round(bps / HBM_PEAK, 4),
            "pil_images_per_s_one_core": None if pil is None else round(pil, 1),
            "torch_interpolate_ms": round(tms, 3), "torch_interpolate_images_per_s": round(N / (tms * 1e-3))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--images", type=int, default=256)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_preprocess.py needs the GPU: there is nothing to time without it")
    imgs = _images(a.images)
    res = {"bench": "preprocess_images", "device": torch.cuda.get_device_name(0), "hbm_peak_bytes_per_s": HBM_PEAK,
           "cases": [case(imgs, S, a.reps, a.iters) for S in (224, 448)]}
    line = json.dumps(res)
    os.makedirs(a.out_dir, exist_ok=True)
    with open(os.path.join(a.out_dir, "preprocess_bench.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
