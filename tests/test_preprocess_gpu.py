"""GPU: dl_vqa_amd.preprocess_images against the PIL-made fixtures (tests/golden/preprocess.npz), bit for bit.  Every
comparison is torch.equal with a fixture, never with the kernel's own output; the inputs are recomputed from
tests/preprocess_ref.synthetic_image."""
import numpy as np
import pytest
import torch

from tests import preprocess_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _run(names, **kw):
    from dl_vqa_amd import preprocess_images
    S, cf = R.case_args(names[0])
    out = preprocess_images([R.case_image(n) for n in names], S, central_fraction=cf, device=DEV, **kw)
    torch.cuda.synchronize()
    return out


# 37 x 53 / 53 x 37 -> 16 (non-integer down-scale, the short side either way); 20 x 20 -> 32 (up-scale); 64 x 64 -> 64 (both
# passes skipped); 100 x 64 -> 64 (vertical only); 33 x 100 -> 16 at cf = 16/24 (window strictly inside); 480 x 640 -> 32
# (scale 15: the widest band of source rows); S = 18 (no band height divides it); then the sizes of the five-image batch and
# the crop offset that rounds up
@pytest.mark.parametrize("name", list(R.CASES))
def test_single_image_equals_fixture(name):
    out = _run([name])
    S = R.CASES[name][2]
    assert out.is_cuda and out.dtype == torch.float16 and tuple(out.shape) == (1, 3, S, S) and out.is_contiguous()
    assert torch.equal(out[0].cpu(), R.golden()[name])


def test_five_sizes_in_one_call_any_order():
    g = R.golden()
    want = torch.stack([g[n] for n in R.BATCH5])
    assert len({R.CASES[n][:2] for n in R.BATCH5}) == 5
    out = _run(R.BATCH5)
    assert torch.equal(out.cpu(), want)                           # what the five single-image calls give (the fixtures)
    rev = _run(R.BATCH5[::-1])
    assert torch.equal(rev.cpu().flip(0), want)                   # the list reversed, un-reversed afterwards


def test_out_dtype_float32():
    out = _run([R.F32_CASE], out_dtype=torch.float32)
    assert out.dtype == torch.float32 and torch.equal(out[0].cpu(), R.golden()[R.F32_CASE + "/f32"])


def test_device_resident_non_contiguous_and_mixed_inputs():
    from dl_vqa_amd import preprocess_images
    g = R.golden()
    a, b = R.case_image("down_37x53"), R.case_image("down_53x37")
    # a device image that is a strided window of a larger tensor (neither rows nor pixels are dense)
    big = torch.zeros(40, 2 * 53 + 3, 4, dtype=torch.uint8, device=DEV)
    big[2:39, 1:107:2, :3] = torch.from_numpy(a).to(DEV)
    view = big[2:39, 1:107:2, :3]
    assert not view.is_contiguous() and tuple(view.shape) == (37, 53, 3)
    out = preprocess_images([view], 16)                           # the device is implied by the image
    assert out.device == view.device and torch.equal(out[0].cpu(), g["down_37x53"])
    # host and device images in one list, one of them a non-contiguous numpy view
    bn = np.zeros((53, 37, 4), dtype=np.uint8)
    bn[:, :, :3] = b
    out = preprocess_images([bn[:, :, :3], view, torch.from_numpy(b)], 16)
    assert torch.equal(out.cpu(), torch.stack([g["down_53x37"], g["down_37x53"], g["down_53x37"]]))
    # one [N, H, W, 3] tensor: on the device (read in place) and on the host
    both = torch.from_numpy(np.stack([a, a]))
    want = torch.stack([g["down_37x53"], g["down_37x53"]])
    assert torch.equal(preprocess_images(both.to(DEV), 16).cpu(), want)
    assert torch.equal(preprocess_images(both, 16, device=DEV).cpu(), want)
    assert torch.equal(preprocess_images(both.numpy(), 16, device=DEV).cpu(), want)
    empty = preprocess_images([], 16, device=DEV)
    assert tuple(empty.shape) == (0, 3, 16, 16) and empty.dtype == torch.float16 and empty.is_cuda


def _tiny_cfg():
    # the first block with 32 output channels: the dedicated first-conv kernels, which read fp16 images as they are
    return {
        "text": {"question_features": 16, "embedding_features": 12, "dropout": 0.3, "num_lstm_layers": 1, "bidirectional": True},
        "image": {"kernel_size": 3, "dropout": 0.3, "num_channels": [3, 32, 16, 32], "stride": 1, "do_skip_connection": False},
        "attention": {"hidden_dim": 24, "glimpses": 2, "do_option": "+", "dropout": 0.3},
        "classifier": {"hidden_dim": 20, "dropout": 0.3},
        "max_answers": 12,
    }


def test_end_to_end_into_encode_images_and_predict(monkeypatch):
    from dl_vqa_amd import VqaNet, ops, preprocess_images
    g = R.golden()
    names = ["up_20x20", "big_480x640"]                           # both to S = 32
    V = 30
    torch.manual_seed(3)
    m = VqaNet(_tiny_cfg(), V).to(DEV).eval()
    assert ops.conv0_supported(3, 32, 32, 32, 1)
    q = torch.tensor([[3, 7, 1, 0, 0], [9, 2, 4, 6, 5], [8, 1, 0, 0, 0]], device=DEV)
    q_len = torch.tensor([3, 5, 2], device=DEV)
    img = [0, 1, 1]

    def boom(*a, **k):
        raise AssertionError("vqa_half_to_float must not run: the fp16 result is read as it is")
    monkeypatch.setattr(ops, "half_to_float", boom)

    v = preprocess_images([R.case_image(n) for n in names], 32, device=DEV)
    v_ref = torch.stack([g[n] for n in names]).to(DEV)            # the fixture tensor uploaded from the host
    assert v.dtype == torch.float16 and torch.equal(v, v_ref)
    f, f_ref = m.encode_images(v), m.encode_images(v_ref)
    assert torch.equal(f.vn, f_ref.vn) and torch.equal(f.vprime, f_ref.vprime) and f.grid == f_ref.grid
    top, top_ref = m.predict(f, q, q_len, img, k=3), m.predict(f_ref, q, q_len, img, k=3)
    assert torch.equal(top.indices, top_ref.indices) and torch.equal(top.probs, top_ref.probs)
    with torch.no_grad():
        y, y_ref = m(v[img], q, q_len), m(v_ref[img], q, q_len)   # forward on the fp16 result, no widening pass
    torch.cuda.synchronize()
    assert torch.equal(y, y_ref) and bool(torch.isfinite(y).all())
