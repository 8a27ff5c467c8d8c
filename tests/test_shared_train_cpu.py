"""CPU: training through shared image features (VqaNet.forward_shared / train.run_batch_shared) -- the new entry points in
the header, the ctypes prototypes and the built library, their host-side argument validation, and the errors the public
calls raise before any device work."""
import re

import pytest
import torch

from dl_vqa_amd import VqaNet
from tests.golden_util import Golden, full_cfg, tiny_cfg

NEW_ENTRY_POINTS = ("vqa_att_score_grouped_drop_fwd", "vqa_att_apply_gather_bwd", "vqa_att_score_grouped_bwd")


def test_new_entry_points_in_header_prototypes_and_library():
    from dl_vqa_amd import _lib, build
    build.build_library(verbose=False)
    with open(_lib.HEADER_PATH) as f:
        header = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    assert _lib.header_abi_version() == 9                      # 9 since vqa_conv3x3_x3_plan; additions before it kept 8
    for name in NEW_ENTRY_POINTS + ("vqa_att_score_grouped_tiles",):
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in _lib.PROTOTYPES, name
    lib = _lib.load()
    assert lib.vqa_abi_version() == 9
    for name in NEW_ENTRY_POINTS + ("vqa_att_score_grouped_tiles",):
        assert hasattr(lib, name), name
    assert [lib.vqa_att_score_grouped_tiles(P) for P in (1, 16, 17, 676)] == [1, 1, 2, 43]


def test_grouped_drop_score_argument_validation_without_gpu():
    """vprime, qp, wx, wx_ld, bx, order, offsets, score, N, B, P, mid, G, mode, p, seed, stream (pointers are made-up
    16-byte-aligned integers: every check runs on the host before any HIP call, nothing dereferences them)."""
    from dl_vqa_amd import _lib
    lib = _lib.load()
    f = lib.vqa_att_score_grouped_drop_fwd
    err = lib.vqa_last_error
    assert f(16, 16, 16, 8, 16, 16, 16, 16, 2, 3, 4, 8, 9, 0, 0.3, 1, None) == 1 and b"glimpses" in err()        # G = 9
    assert f(16, 16, 16, 8, 16, 16, 16, 16, 2, 3, 4, 6, 2, 0, 0.3, 1, None) == 1 and b"mid=6" in err()           # mid = 6
    assert f(16, 16, 16, 8, 16, 16, 16, 16, 2, 3, 4, 8, 2, 3, 0.3, 1, None) == 1 and b"mode 3" in err()          # mode = 3
    assert f(None, 16, 16, 8, 16, 16, 16, 16, 2, 3, 4, 8, 2, 0, 0.3, 1, None) == 1 and b"null pointer" in err()
    assert f(16, 16, 16, 8, 16, None, 16, 16, 2, 3, 4, 8, 2, 0, 0.3, 1, None) == 1 and b"order" in err()
    assert f(16, 16, 16, 8, 16, 16, None, 16, 2, 3, 4, 8, 2, 0, 0.3, 1, None) == 1 and b"offsets" in err()
    assert f(16, 16, 16, 8, 16, 16, 16, 16, 0, 3, 4, 8, 2, 0, 0.3, 1, None) == 1 and b"out of range" in err()    # N = 0
    assert f(16, 16, 16, 8, 16, 16, 16, 16, 2, 3, 4, 8, 2, 2, 0.3, 1, None) == 1 and b"wx_ld" in err()           # '|': wx_ld < 2 mid
    assert f(16, 16, 16, 8, 16, 16, 16, 16, 2, 3, 4, 8, 2, 0, 1.0, 1, None) == 1 and b"p=1" in err()             # p = 1
    assert f(16, 16, 16, 8, 16, 16, 16, 16, 2, 3, 4, 8, 2, 0, -0.5, 1, None) == 1 and b"p=-0.5" in err()         # p < 0
    assert f(20, 16, 16, 8, 16, 16, 16, 16, 2, 3, 4, 8, 2, 0, 0.3, 1, None) == 1 and b"aligned" in err()
    assert f(16, 16, 16, 8, 16, 16, 16, 16, 2, 0, 4, 8, 2, 0, 0.3, 1, None) == 0                                 # B = 0: no launch


def test_apply_gather_bwd_argument_validation_without_gpu():
    """dout, dout_ld, probs, vn, img, order, offsets, dscore, dvn, dscore_rowsum, N, B, P, C, G, stream."""
    from dl_vqa_amd import _lib
    lib = _lib.load()
    f = lib.vqa_att_apply_gather_bwd
    err = lib.vqa_last_error
    assert f(None, 64, 16, 16, 16, 16, 16, 16, 16, 16, 2, 3, 4, 8, 2, None) == 1 and b"null pointer" in err()
    assert f(16, 64, 16, 16, 16, 16, 16, 16, None, 16, 2, 3, 4, 8, 2, None) == 1 and b"null pointer" in err()    # dvn is required
    assert f(16, 64, 16, 16, None, 16, 16, 16, 16, 16, 2, 3, 4, 8, 2, None) == 1 and b"img" in err()
    assert f(16, 64, 16, 16, 16, None, 16, 16, 16, 16, 2, 3, 4, 8, 2, None) == 1 and b"order" in err()
    assert f(16, 64, 16, 16, 16, 16, None, 16, 16, 16, 2, 3, 4, 8, 2, None) == 1 and b"offsets" in err()
    assert f(16, 64, 16, 16, 16, 16, 16, 16, 16, 16, 2, 3, 4, 8, 9, None) == 1 and b"glimpses" in err()          # G = 9
    assert f(16, 64, 16, 16, 16, 16, 16, 16, 16, 16, 0, 3, 4, 8, 2, None) == 1 and b"out of range" in err()      # N = 0
    assert f(16, 64, 16, 16, 16, 16, 16, 16, 16, 16, 2, 3, 4, 6, 2, None) == 1 and b"C=6" in err()               # C % 4
    assert f(16, 8, 16, 16, 16, 16, 16, 16, 16, 16, 2, 3, 4, 8, 2, None) == 1 and b"dout_ld=8" in err()          # dout_ld < G*C
    assert f(16, 64, 16, 20, 16, 16, 16, 16, 16, 16, 2, 3, 4, 8, 2, None) == 1 and b"aligned" in err()
    assert f(16, 64, 16, 16, 16, 16, 16, 16, 16, None, 2, 0, 4, 8, 2, None) == 0                                 # B = 0: no launch


def test_grouped_score_bwd_argument_validation_without_gpu():
    """dscore, vprime, qp, wx, wx_ld, order, offsets, dvprime, dq_part, dwx_part, N, B, P, mid, G, mode, p, seed, stream."""
    from dl_vqa_amd import _lib
    lib = _lib.load()
    f = lib.vqa_att_score_grouped_bwd
    err = lib.vqa_last_error
    ok = (16, 16, 16, 16, 8, 16, 16, 16, 16, 16, 2, 3, 4, 8, 2, 0, 0.3, 1, None)

    def call(**ch):
        a = list(ok)
        names = ("dscore", "vprime", "qp", "wx", "wx_ld", "order", "offsets", "dvprime", "dq_part", "dwx_part", "N", "B", "P",
                 "mid", "G", "mode", "p", "seed", "stream")
        for k, val in ch.items():
            a[names.index(k)] = val
        return f(*a)

    assert call(G=9) == 1 and b"glimpses" in err()
    assert call(mid=6) == 1 and b"mid=6" in err()
    assert call(mode=3) == 1 and b"mode 3" in err()
    assert call(N=0) == 1 and b"out of range" in err()
    assert call(mode=2) == 1 and b"wx_ld" in err()                 # '|': wx_ld = 8 < 2 * mid
    assert call(wx_ld=6, mid=4) == 1 and b"wx_ld" in err()         # wx_ld % 4
    assert call(mid=8192, wx_ld=8192) == 1 and b"mid=8192" in err()
    assert call(p=1.0) == 1 and b"p=1" in err()
    assert call(p=-0.25) == 1 and b"p=-0.25" in err()
    for name in ("dscore", "vprime", "qp", "wx", "dvprime", "dq_part", "dwx_part"):
        assert call(**{name: None}) == 1 and b"null pointer" in err(), name
    assert call(order=None) == 1 and b"order" in err()
    assert call(offsets=None) == 1 and b"offsets" in err()
    assert call(dvprime=20) == 1 and b"aligned" in err()
    assert call(B=0) == 0                                          # no launch


def test_forward_shared_refuses_bf16_data_parallel_and_cpu_tensors_before_device_work():
    v = torch.zeros(1, 3, 32, 32)
    q, ql = torch.ones(2, 3, dtype=torch.int64), torch.tensor([3, 3])
    m = VqaNet(full_cfg(16), 30, compute_dtype="bf16")              # on the CPU, train mode
    with pytest.raises(NotImplementedError, match="compute_dtype"):
        m.forward_shared(v, q, ql, [0, 0])
    m.eval()
    with pytest.raises(NotImplementedError, match="compute_dtype"):
        m.forward_shared(v, q, ql, [0, 0])
    g = Golden("tiny_plus")
    m = VqaNet(tiny_cfg(g.meta), g.meta["V"])
    m._grad_sync = object()                                         # what distributed.DataParallel sets
    with pytest.raises(NotImplementedError, match="data-parallel"):
        m.forward_shared(v, q, ql, [0, 0])
    m._grad_sync = None
    for mode in (m.train, m.eval):                                  # both modes are served: the device check speaks
        mode()
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            m.forward_shared(v, q, ql, [0, 0])
    assert m._last_ctx is None and m._flat_param is None and len(m._pending) == 0


def test_run_batch_shared_rejects_an_image_index_of_the_wrong_length():
    from dl_vqa_amd.train import run_batch_shared
    g = Golden("tiny_plus")
    m = VqaNet(tiny_cfg(g.meta), g.meta["V"])
    batch = (g.t["v"][:2], g.t["q"], g.t["a_idx"], g.t["a_val"], g.t["a_len"], torch.arange(3), g.t["q_len"])
    for bad in ([0, 1], [0, 1, 1, 0], torch.tensor([1])):
        with pytest.raises(ValueError, match="image_index entries for 3 questions"):
            run_batch_shared(m, batch, 12, bad)
