"""CPU: the host side of the grouped paths' index handling (dl_vqa_amd.model) -- an image index is converted to the host
once and that tensor is handed on, and the index tensors of a call go to the device as views of ONE uploaded tensor."""
import pytest
import torch

from dl_vqa_amd import compact_image_index, group_by_image
from dl_vqa_amd.model import _host_image_index, _upload_index

# (B, N, image_index): one question; an image nobody asks about; repeats
CASES = ((1, 1, [0]), (3, 4, [3, 0, 2]), (5, 2, [1, 1, 0, 1, 0]))


@pytest.mark.parametrize("B,N,image_index", CASES)
def test_upload_returns_int32_views_of_one_tensor(B, N, image_index):
    img = _host_image_index(image_index, N)
    order, offsets = group_by_image(img, N)
    rows, slot, order_u, offsets_u = compact_image_index(img, N)
    qrow = torch.arange(B, dtype=torch.int64).flip(0)
    for parts in ((order, offsets, img), (order, offsets, img, qrow), (rows, order_u, offsets_u, img)):
        views = _upload_index("cpu", *parts)
        assert len(views) == len(parts)
        for got, want in zip(views, parts):
            assert got.dtype == torch.int32 and got.shape == want.shape
            assert torch.equal(got.long(), want.long())
        # the single-copy check: every view lies in the one tensor that was moved, one behind the other
        base = views[0].untyped_storage().data_ptr()
        assert all(t.untyped_storage().data_ptr() == base for t in views)
        assert views[0].untyped_storage().nbytes() == 4 * sum(p.numel() for p in parts)
        at = 0
        for t in views:
            assert t.storage_offset() == at
            at += t.numel()
    assert order.numel() == B and offsets.numel() == N + 1 and rows.numel() <= N


@pytest.mark.parametrize("B,N,image_index", CASES)
def test_a_converted_index_passes_through_without_a_copy(B, N, image_index):
    img = _host_image_index(image_index, N)
    assert img.dtype == torch.int64 and img.device.type == "cpu" and img.tolist() == image_index
    again = _host_image_index(img, N)
    assert again.data_ptr() == img.data_ptr() and again.shape == img.shape         # the same memory: nothing converted
    for src in (image_index, torch.tensor(image_index, dtype=torch.int32), torch.tensor(image_index).reshape(B, 1)):
        assert torch.equal(_host_image_index(src, N), img)
    # compact_image_index and group_by_image: the same tensors from the converted index as from the caller's list
    for got, want in zip(compact_image_index(img, N), compact_image_index(image_index, N)):
        assert got.dtype == want.dtype == torch.int32 and torch.equal(got, want)
    for got, want in zip(group_by_image(img, N), group_by_image(image_index, N)):
        assert got.dtype == want.dtype == torch.int32 and torch.equal(got, want)


@pytest.mark.parametrize("B,N,image_index", CASES)
def test_out_of_range_entries_still_raise(B, N, image_index):
    for bad in (-1, N):
        idx = image_index[:-1] + [bad]
        for given in (idx, torch.tensor(idx), _host_image_index(image_index, N).clone().index_fill_(0, torch.tensor([B - 1]), bad)):
            with pytest.raises(IndexError, match=rf"image_index entry {bad} out of range \[0, {N}\)"):
                group_by_image(given, N)
            with pytest.raises(IndexError, match=rf"image_index entry {bad} out of range \[0, {N}\)"):
                compact_image_index(given, N)


def test_question_index_keeps_its_message():
    with pytest.raises(IndexError, match=r"question_index entry 2 out of range \[0, 2\) \(2 encoded questions\)"):
        _host_image_index([0, 2], 2, "question_index", "questions")
    with pytest.raises(IndexError, match=r"question_index entry -1 out of range \[0, 2\) \(2 encoded questions\)"):
        _host_image_index(torch.tensor([1, -1]), 2, "question_index", "questions")
