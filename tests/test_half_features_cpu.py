"""CPU: float16 image-feature caches -- the API errors that need no device, the header's append-only record of the new entry
points, and the host-side argument validation of every one of them.  Pointers are made-up integers with the alignment a case
needs: every check runs on the host before any HIP call, nothing dereferences them (tests/test_att_apply_args_cpu.py)."""
import os
import re

import pytest
import torch

from dl_vqa_amd import ImageFeatures, VqaNet
from tests.golden_util import Golden, tiny_cfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vqa_float_to_half", "vqa_gather_rows_drop_f16", "vqa_att_apply_gather_fwd_f16", "vqa_att_apply_gather_dscore_f16",
       "vqa_att_score_grouped_fwd_f16", "vqa_att_score_grouped_pairs_fwd_f16")


def _caller(f, names, ok):
    def call(**ch):
        a = list(ok)
        for k, val in ch.items():
            a[names.index(k)] = val
        return f(*a)
    return call


def _lib():
    from dl_vqa_amd import _lib
    lib = _lib.load()
    return lib, lib.vqa_last_error


# ----------------------------------------------------------------------------- API
def _tiny():
    g = Golden("tiny_plus")
    m = VqaNet(tiny_cfg(g.meta), g.meta["V"])
    m.load_state_dict(g.sd)
    return m.eval()


def test_encode_images_refuses_other_dtypes_before_any_device_work():
    m = _tiny()                                                       # a host model: any device work would raise RuntimeError
    v = torch.zeros(1, 3, 16, 16)
    for bad in (torch.bfloat16, torch.float64, torch.int8, None, "float16"):
        with pytest.raises(ValueError, match="torch.float32 or torch.float16"):
            m.encode_images(v, dtype=bad)
    m.train()                                                         # ... and before the mode check
    with pytest.raises(ValueError, match="torch.float32 or torch.float16"):
        m.encode_images(v, dtype=torch.bfloat16)


def test_image_features_dtype_cat_and_to_on_host_holders():
    m = _tiny()
    eng = m._engine
    m._flat_param = torch.zeros(4)                                    # stands in for the flat buffer (ownership marks)
    mk = lambda n, dt, vp=True: ImageFeatures(torch.zeros(n, 4, eng.C, dtype=dt),
                                              torch.zeros(n * 4, eng.mid, dtype=dt) if vp else None, (2, 2), m)
    a, b, c = mk(2, torch.float16), mk(3, torch.float16), mk(1, torch.float32)
    assert a.dtype == torch.float16 and c.dtype == torch.float32
    both = ImageFeatures.cat([a, b])
    assert both.dtype == torch.float16 and both.N == 5 and both.vprime.dtype == torch.float16
    assert ImageFeatures.cat([mk(2, torch.float16, vp=False), b]).vprime is None
    with pytest.raises(ValueError, match="storage formats"):
        ImageFeatures.cat([a, c])
    with pytest.raises(ValueError, match="storage formats"):
        ImageFeatures.cat([c, a, b])
    assert a.to(torch.float16) is a and c.to(torch.float32) is c      # the same dtype: no copy, no device
    for bad in (torch.bfloat16, torch.float64):
        with pytest.raises(ValueError, match="torch.float32 or torch.float16"):
            a.to(bad)


# ----------------------------------------------------------------------------- header
def test_header_lists_the_new_entry_points_append_only_at_abi_9():
    from dl_vqa_amd import _lib
    text = open(os.path.join(ROOT, "include", "vqa_hip.h")).read()
    head = text[:text.index("#define VQA_ABI_VERSION")]
    comment = head[head.rindex("/*"):]                                # the comment that records every appended entry point
    assert "append-only" in comment
    for name in NEW:
        assert name in comment, name
        assert name in _lib.PROTOTYPES, name
    # appended: declared behind the last entry point of the parent's header, in the order of the comment
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    order = re.findall(r"\b(vqa_[a-z0-9_]+)\s*\(", code)
    assert tuple(order[-len(NEW):]) == NEW and order[-len(NEW) - 1] == "vqa_conv3x3_x3_plan"
    assert _lib.header_abi_version() == 9 and _lib.load().vqa_abi_version() == 9


# ----------------------------------------------------------------------------- host argument validation
def test_float_to_half_argument_validation_without_gpu():
    lib, err = _lib()
    call = _caller(lib.vqa_float_to_half, ("x", "y", "n", "stream"), (16, 32, 100, None))
    for name in ("x", "y"):
        assert call(**{name: None}) == 1 and b"bad args" in err(), name
        assert call(**{name: 24}) == 1 and b"16-byte aligned" in err(), name
    assert call(n=-1) == 1 and b"bad args" in err()
    assert call(n=0) == 0                                             # no launch


def test_gather_rows_drop_f16_argument_validation_without_gpu():
    lib, err = _lib()
    names = ("src", "rows", "dst", "n", "M", "row_len", "p", "seed", "stream")
    call = _caller(lib.vqa_gather_rows_drop_f16, names, (16, 16, 16, 3, 5, 8, 0.0, 1, None))
    for name in ("src", "rows", "dst"):
        assert call(**{name: None}) == 1 and b"null pointer" in err(), name
    assert call(n=-1) == 1 and b"out of range" in err()
    assert call(M=0) == 1 and b"out of range" in err()
    assert call(row_len=0) == 1 and b"out of range" in err()
    assert call(p=1.0) == 1 and b"outside [0, 1)" in err()
    assert call(p=-0.5) == 1 and b"outside [0, 1)" in err()
    assert call(src=17, n=0) == 1 and b"aligned" in err()             # no half starts at an odd address
    assert call(dst=18, n=0) == 1 and b"aligned" in err()
    assert call(n=0) == 0                                             # no launch
    assert call(n=0, src=18, dst=20, row_len=7) == 0                  # misaligned / odd length: served (the scalar path)


def test_apply_gather_fwd_f16_argument_validation_without_gpu():
    lib, err = _lib()
    names = ("score", "vn", "img", "probs", "out", "out_ld", "N", "B", "P", "C", "G", "stream")
    call = _caller(lib.vqa_att_apply_gather_fwd_f16, names, (16, 16, 16, 16, 16, 64, 2, 3, 4, 8, 2, None))
    for name in ("score", "vn", "probs", "out"):
        assert call(**{name: None}) == 1 and b"null pointer" in err(), name
    assert call(img=None) == 1 and b"img" in err()
    assert call(G=0) == 1 and b"glimpses" in err()
    assert call(G=5) == 1 and b"glimpses" in err()
    assert call(P=0) == 1 and b"out of range" in err()
    assert call(N=0) == 1 and b"out of range" in err()
    assert call(B=-1) == 1 and b"out of range" in err()
    assert call(C=0) == 1 and b"out of range" in err()
    assert call(out_ld=8) == 1 and b"out_ld=8" in err()               # out_ld < G*C
    assert call(P=20000) == 1 and b"too large for LDS" in err()
    assert call(vn=17, B=0) == 1 and b"aligned" in err()              # no half starts at an odd address
    assert call(B=0) == 0                                             # no launch
    assert call(B=0, vn=20) == 0                                      # vn at 4 (mod 8): served (the scalar kernel)
    assert call(B=0, vn=18, C=6) == 0                                 # odd width: served


def test_apply_gather_dscore_f16_argument_validation_without_gpu():
    lib, err = _lib()
    names = ("dout", "dout_ld", "probs", "vn", "img", "dscore", "rowsum", "N", "B", "P", "C", "G", "stream")
    call = _caller(lib.vqa_att_apply_gather_dscore_f16, names, (16, 64, 16, 16, 16, 16, 16, 2, 3, 4, 8, 2, None))
    for name in ("dout", "probs", "vn", "dscore"):
        assert call(**{name: None}) == 1 and b"null pointer" in err(), name
    assert call(img=None) == 1 and b"img" in err()
    assert call(G=0) == 1 and b"glimpses" in err()
    assert call(G=5) == 1 and b"glimpses" in err()
    assert call(P=0) == 1 and b"out of range" in err()
    assert call(N=0) == 1 and b"out of range" in err()
    assert call(C=6) == 1 and b"C=6" in err()                         # C % 4
    assert call(dout_ld=8) == 1 and b"dout_ld=8" in err()             # dout_ld < G*C
    assert call(dout_ld=18) == 1 and b"dout_ld=18" in err()           # dout_ld % 4
    assert call(B=0, vn=20) == 1 and b"8-byte aligned" in err()       # a half vn at 4 (mod 8): refused
    assert call(B=0, vn=24) == 0                                      # at 8 (mod 16): a quad of halves is 8 bytes
    assert call(B=0, dout=24) == 1 and b"16-byte aligned" in err()    # the fp32 operand at 8 (mod 16): refused
    assert call(B=0) == 0                                             # no launch
    assert call(B=0, rowsum=None, P=20000) == 0                       # rowsum is optional; no LDS bound in the backward


@pytest.mark.parametrize("pairs", [False, True])
def test_score_grouped_f16_argument_validation_without_gpu(pairs):
    lib, err = _lib()
    if pairs:
        names = ("vprime", "qp", "qrow", "wx", "wx_ld", "bx", "order", "offsets", "score", "N", "B", "M", "P", "mid", "G", "mode",
                 "stream")
        call = _caller(lib.vqa_att_score_grouped_pairs_fwd_f16, names, (16, 16, 16, 16, 256, 16, 16, 16, 16, 2, 3, 2, 4, 256, 2, 0,
                                                                        None))
        assert call(qrow=None) == 1 and b"null qrow" in err()
        assert call(M=0) == 1 and b"question rows" in err()
    else:
        names = ("vprime", "qp", "wx", "wx_ld", "bx", "order", "offsets", "score", "N", "B", "P", "mid", "G", "mode", "stream")
        call = _caller(lib.vqa_att_score_grouped_fwd_f16, names, (16, 16, 16, 256, 16, 16, 16, 16, 2, 3, 4, 256, 2, 0, None))
    for name in ("vprime", "qp", "wx", "bx", "score"):
        assert call(**{name: None}) == 1 and b"null pointer" in err(), name
    for name in ("order", "offsets"):
        assert call(**{name: None}) == 1 and b"null order / offsets" in err(), name
    assert call(G=0) == 1 and b"glimpses" in err()
    assert call(G=5) == 1 and b"glimpses" in err()
    assert call(mode=3) == 1 and b"mode 3" in err()
    assert call(P=0) == 1 and b"out of range" in err()
    assert call(N=0) == 1 and b"out of range" in err()
    assert call(N=65536) == 1 and b"out of range" in err()
    assert call(mid=6) == 1 and b"multiples of 4" in err()
    assert call(wx_ld=128) == 1 and b"wx_ld" in err()                 # wx_ld < mid
    assert call(mode=2) == 1 and b"wx_ld" in err()                    # '|' needs 2 * mid weights per glimpse
    assert call(mid=8192, wx_ld=8192) == 1 and b"too large" in err()
    assert call(B=0, vprime=20) == 1 and b"8-byte aligned" in err()   # a half v' at 4 (mod 8): refused
    assert call(B=0, vprime=24) == 0                                  # at 8 (mod 16): a quad of halves is 8 bytes
    for name in ("qp", "wx"):
        assert call(B=0, **{name: 24}) == 1 and b"16-byte aligned" in err(), name     # the fp32 operands at 8 (mod 16)
    assert call(B=0) == 0                                             # no launch
