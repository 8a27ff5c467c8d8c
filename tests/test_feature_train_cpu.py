"""CPU: training on cached image features (VqaNet.forward_features / train.run_batch_features) -- the two new entry points in
the header, the ctypes prototypes and the built library, their host-side argument validation, compact_image_index against
its definition, and the errors the public calls raise before any device work."""
import re

import pytest
import torch

from dl_vqa_amd import ImageFeatures, VqaNet, compact_image_index, group_by_image
from tests.golden_util import Golden, full_cfg, tiny_cfg

NEW_ENTRY_POINTS = ("vqa_gather_rows_drop", "vqa_att_apply_gather_dscore")


def test_feature_entry_points_in_header_prototypes_and_library():
    from dl_vqa_amd import _lib, build
    build.build_library(verbose=False)
    with open(_lib.HEADER_PATH) as f:
        text = f.read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert _lib.header_abi_version() == 9                      # 9 since vqa_conv3x3_x3_plan; additions before it kept 8
    for name in NEW_ENTRY_POINTS:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in _lib.PROTOTYPES, name
        assert name in text.split("#define VQA_ABI_VERSION")[0], name      # listed among the append-only additions
    lib = _lib.load()
    assert lib.vqa_abi_version() == 9
    for name in NEW_ENTRY_POINTS:
        assert hasattr(lib, name), name


def test_gather_rows_drop_argument_validation_without_gpu():
    """src, rows, dst, n, M, row_len, p, seed, stream (pointers are made-up integers: every check runs on the host before
    any HIP call, nothing dereferences them)."""
    from dl_vqa_amd import _lib
    lib = _lib.load()
    f = lib.vqa_gather_rows_drop
    err = lib.vqa_last_error
    assert f(None, 16, 16, 2, 3, 8, 0.3, 1, None) == 1 and b"null pointer" in err()
    assert f(16, None, 16, 2, 3, 8, 0.3, 1, None) == 1 and b"null pointer" in err()
    assert f(16, 16, None, 2, 3, 8, 0.3, 1, None) == 1 and b"null pointer" in err()
    assert f(16, 16, 16, -1, 3, 8, 0.3, 1, None) == 1 and b"n=-1" in err()                # negative n
    assert f(16, 16, 16, 2, 0, 8, 0.3, 1, None) == 1 and b"M=0" in err()
    assert f(16, 16, 16, 2, 3, 0, 0.3, 1, None) == 1 and b"row_len=0" in err()
    assert f(16, 16, 16, 2, 3, 8, 1.0, 1, None) == 1 and b"p=1" in err()                  # p = 1
    assert f(16, 16, 16, 2, 3, 8, -0.5, 1, None) == 1 and b"p=-0.5" in err()              # p < 0
    assert f(16, 16, 16, 0, 3, 8, 0.3, 1, None) == 0                                      # n = 0: no launch
    assert f(20, 16, 18, 0, 3, 7, 0.0, 1, None) == 0                                      # odd length, unaligned: served


def test_apply_gather_dscore_argument_validation_without_gpu():
    """dout, dout_ld, probs, vn, img, dscore, dscore_rowsum, N, B, P, C, G, stream."""
    from dl_vqa_amd import _lib
    lib = _lib.load()
    f = lib.vqa_att_apply_gather_dscore
    err = lib.vqa_last_error
    ok = (16, 64, 16, 16, 16, 16, 16, 2, 3, 4, 8, 2, None)
    names = ("dout", "dout_ld", "probs", "vn", "img", "dscore", "rowsum", "N", "B", "P", "C", "G", "stream")

    def call(**ch):
        a = list(ok)
        for k, val in ch.items():
            a[names.index(k)] = val
        return f(*a)

    for name in ("dout", "probs", "vn", "dscore"):
        assert call(**{name: None}) == 1 and b"null pointer" in err(), name
    assert call(img=None) == 1 and b"img" in err()
    assert call(G=9) == 1 and b"glimpses" in err()                 # G outside 1..4
    assert call(G=0) == 1 and b"glimpses" in err()
    assert call(N=0) == 1 and b"out of range" in err()
    assert call(B=-1) == 1 and b"out of range" in err()
    assert call(C=6) == 1 and b"C=6" in err()                      # C % 4
    assert call(dout_ld=8) == 1 and b"dout_ld=8" in err()          # dout_ld < G*C
    assert call(vn=20) == 1 and b"aligned" in err()
    assert call(rowsum=None, B=0) == 0                             # B = 0: no launch; the row sums are optional


def _check_compact(idx, N):
    rows, slot, order, offsets = compact_image_index(idx, N)
    t = torch.as_tensor(idx).reshape(-1).to(torch.int64)
    want_rows = sorted(set(t.tolist()))
    assert rows.dtype == slot.dtype == order.dtype == offsets.dtype == torch.int32
    assert rows.tolist() == want_rows                                          # distinct, ascending
    assert slot.shape == t.shape and torch.equal(rows.long()[slot.long()], t)  # rows[slot[b]] == image_index[b]
    o2, f2 = group_by_image(slot, len(want_rows))
    assert torch.equal(order, o2) and torch.equal(offsets, f2)
    assert offsets.numel() == len(want_rows) + 1 and int(offsets[-1]) == t.numel()
    for n in range(len(want_rows)):                                            # every asked row has a question; stable order
        members = order[int(offsets[n]):int(offsets[n + 1])].tolist()
        assert members and members == [b for b in range(t.numel()) if int(t[b]) == want_rows[n]]
    return rows


def test_compact_image_index_matches_its_definition():
    g = torch.Generator().manual_seed(11)
    for N, B in ((1, 1), (5, 7), (50, 9), (2048, 256), (3, 40)):
        _check_compact(torch.randint(0, N, (B,), generator=g), N)
    assert _check_compact([4, 4, 4], 9).tolist() == [4]                        # a single image
    assert _check_compact(torch.randperm(16, generator=g), 16).tolist() == list(range(16))      # all rows distinct
    assert 0 not in _check_compact([3, 1, 3, 2, 1], 4).tolist()                # row 0 nobody asks about
    assert _check_compact(torch.tensor([2, 0], dtype=torch.int32), 3).tolist() == [0, 2]
    rows, slot, order, offsets = compact_image_index([], 4)                    # empty: empty arrays, offsets [0]
    assert rows.numel() == slot.numel() == order.numel() == 0 and offsets.tolist() == [0]
    for bad in ([0, 4], [-1, 2], torch.tensor([7])):
        with pytest.raises(IndexError, match=r"out of range \[0, 4\)"):
            compact_image_index(bad, 4)


def _fake_feats(vn):
    """An ImageFeatures holder around a CPU tensor, built without a model: what the checks that precede any device work see."""
    f = object.__new__(ImageFeatures)
    f.vn, f.vprime, f.grid, f.N = vn, None, (2, 2), vn.shape[0]
    f._model, f._flat_ptr = (lambda: None), 0
    return f


def test_forward_features_refuses_bf16_data_parallel_wrong_feats_and_cpu_tensors_before_device_work():
    q, ql = torch.ones(2, 3, dtype=torch.int64), torch.tensor([3, 3])
    m = VqaNet(full_cfg(16), 30, compute_dtype="bf16")              # on the CPU, train mode
    feats = _fake_feats(torch.zeros(1, 4, 256))
    for mode in (m.train, m.eval):
        mode()
        with pytest.raises(NotImplementedError, match="compute_dtype"):
            m.forward_features(feats, q, ql, [0, 0])
    g = Golden("tiny_plus")
    m = VqaNet(tiny_cfg(g.meta), g.meta["V"])
    m._grad_sync = object()                                         # what distributed.DataParallel sets
    with pytest.raises(NotImplementedError, match="data-parallel"):
        m.forward_features(feats, q, ql, [0, 0])
    m._grad_sync = None
    for wrong in (torch.zeros(1, 4, 8), None, (torch.zeros(1, 4, 8), None)):
        with pytest.raises(TypeError, match="encode_images"):
            m.forward_features(wrong, q, ql, [0, 0])
    for mode in (m.train, m.eval):                                  # both modes are served: the device check speaks
        mode()
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            m.forward_features(feats, q, ql, [0, 0])
    assert m._last_ctx is None and m._flat_param is None and len(m._pending) == 0


def test_run_batch_features_rejects_an_image_index_of_the_wrong_length():
    from dl_vqa_amd.train import run_batch_features
    g = Golden("tiny_plus")
    m = VqaNet(tiny_cfg(g.meta), g.meta["V"])
    batch = (None, g.t["q"], g.t["a_idx"], g.t["a_val"], g.t["a_len"], torch.arange(3), g.t["q_len"])
    for bad in ([0, 1], [0, 1, 1, 0], torch.tensor([1])):
        with pytest.raises(ValueError, match="image_index entries for 3 questions"):
            run_batch_features(m, batch, 12, _fake_feats(torch.zeros(2, 4, 8)), bad)


def test_image_features_cat_checks_its_parts_on_the_host():
    with pytest.raises(ValueError, match="nothing"):
        ImageFeatures.cat([])
    with pytest.raises(TypeError, match="encode_images"):
        ImageFeatures.cat([torch.zeros(1, 4, 8)])


def test_integration_bank_recipe_numbers_the_rows_in_encoding_order():
    """The index construction of INTEGRATION's bank recipe, run as it is written there: the lines that fill `row_of` are
    taken from the document and executed over chunks of uneven sizes.  Image k of the data set, in encoding order, must get
    bank row k -- the row ImageFeatures.cat gives its features."""
    import os
    doc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "INTEGRATION.md")
    with open(doc) as f:
        blocks = re.findall(r"```python\n(.*?)```", f.read(), flags=re.S)
    block = next(b for b in blocks if "row_of" in b and "run_batch_features" in b)
    lines = block.splitlines()
    start = next(i for i, ln in enumerate(lines) if ln.startswith("for ids, v in image_chunks"))
    body = []
    for ln in lines[start + 1:]:                                   # the loop's body, the lines that build the index
        if not ln.startswith("    "):
            break
        if "row_of" in ln:
            body.append(ln.split("#")[0].rstrip())
    assert any("row_of.update" in ln for ln in body), body
    chunks = [["a", "b", "c"], ["d", "e"], ["f"], ["g", "h", "i", "j"]]
    env = {"row_of": {}, "image_chunks": [(ids, None) for ids in chunks]}
    exec("for ids, v in image_chunks:\n" + "\n".join(body), env)
    flat = [im for ids in chunks for im in ids]
    assert env["row_of"] == {im: k for k, im in enumerate(flat)}
