"""Writes tests/golden/preprocess.npz: the expected outputs of image preprocessing, made with PIL itself.

Run by hand (python tests/golden/make_golden_preprocess.py), never at test time.  For every case of
tests/preprocess_ref.CASES the input is preprocess_ref.synthetic_image (the tests recompute it), and the expected output is
what the reference's transform chain gives for it (preprocessing/preprocess_images.py:8-15,50-52), replayed here from its
statements because torchvision is not a dependency of this repository:
  Resize(R)        short side -> R = int(S / cf), long side int(R * long / short); PIL Image.resize(..., BILINEAR)
  CenterCrop(S)    top = int(round((h - S) / 2.0)), left likewise; PIL Image.crop
  ToTensor         HWC uint8 -> CHW float32, divided by 255
  Normalize        (x - mean) / std per channel in float32
  .astype('float16')
The file holds, per case, "<name>" (float16 [3, S, S]) and "params/<name>" (H, W, S, cf numerator, cf denominator, seed);
"<F32_CASE>/f32" is that case before the last rounding."""
import os
import sys

import numpy as np
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import preprocess_ref as R  # noqa: E402


def reference_pipeline(img_u8, S, cf):
    """float32 [3, S, S] tensor: the chain above on a PIL image."""
    img = Image.fromarray(img_u8, "RGB")
    size = int(S / cf)
    w, h = img.size
    if w <= h:
        ow, oh = size, int(size * h / w)
    else:
        oh, ow = size, int(size * w / h)
    img = img.resize((ow, oh), Image.BILINEAR)
    assert oh >= S and ow >= S, "CenterCrop would pad: not a case of this feature"
    top = int(round((oh - S) / 2.0))
    left = int(round((ow - S) / 2.0))
    img = img.crop((left, top, left + S, top + S))
    t = torch.from_numpy(np.array(img, dtype=np.uint8, copy=True)).permute(2, 0, 1).contiguous()
    t = t.to(torch.float32).div(255)
    mean = torch.tensor(R.MEAN, dtype=torch.float32)
    std = torch.tensor(R.STD, dtype=torch.float32)
    t.sub_(mean[:, None, None]).div_(std[:, None, None])
    return t


def main():
    out = {}
    for name, (H, W, S, (num, den), seed) in R.CASES.items():
        t = reference_pipeline(R.synthetic_image(H, W, seed), S, num / den)
        out[name] = t.numpy().astype("float16")
        out["params/" + name] = np.array([H, W, S, num, den, seed], dtype=np.int32)
        if name == R.F32_CASE:
            out[name + "/f32"] = t.numpy()
    path = os.path.join(HERE, "preprocess.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
