"""CPU: top-k answers (vqa_softmax_topk, dl_vqa_amd.topk_answers, VqaNet.predict) -- the entry point in the header, the
ctypes prototypes and the built library, its host-side argument checks, and the errors the public calls raise before any
device work."""
import re

import pytest
import torch

from tests.golden_util import Golden, full_cfg, tiny_cfg


def test_entry_point_in_header_prototypes_and_library():
    from dl_vqa_amd import _lib, build
    build.build_library(verbose=False)
    with open(_lib.HEADER_PATH) as f:
        header = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    assert re.search(r"\bvqa_softmax_topk\s*\(", header)
    assert "vqa_softmax_topk" in _lib.PROTOTYPES
    lib = _lib.load()
    assert hasattr(lib, "vqa_softmax_topk")
    assert lib.vqa_abi_version() == _lib.header_abi_version() == 9          # 9 since vqa_conv3x3_x3_plan


def test_argument_validation_without_gpu():
    """Every check runs on the host before any HIP call.  Arguments: logits, ld, B, A, k, idx, prob, lse, stream (pointers
    are made-up integers: nothing dereferences them)."""
    from dl_vqa_amd import _lib
    lib = _lib.load()
    f = lib.vqa_softmax_topk
    assert f(16, 12, 3, 12, 0, 16, 16, None, None) == 1 and b"k=0" in lib.vqa_last_error()
    assert f(16, 12, 3, 12, -1, 16, 16, None, None) == 1 and b"k=-1" in lib.vqa_last_error()
    assert f(16, 12, 3, 12, 13, 16, 16, None, None) == 1 and b"k=13" in lib.vqa_last_error()           # k > A
    assert f(16, 3000, 3, 3000, 65, 16, 16, None, None) == 1 and b"k=65" in lib.vqa_last_error()       # k > 64
    assert f(16, 11, 3, 12, 2, 16, 16, None, None) == 1 and b"ld=11" in lib.vqa_last_error()           # ld < A
    assert f(16, 12, 3, 0, 1, 16, 16, None, None) == 1 and b"A=0" in lib.vqa_last_error()
    assert f(16, 12, -1, 12, 1, 16, 16, None, None) == 1 and b"B=-1" in lib.vqa_last_error()
    assert f(16, 12, 3, 12, 2, None, 16, None, None) == 1 and b"null pointer" in lib.vqa_last_error()  # idx
    assert f(16, 12, 3, 12, 2, 16, None, 16, None) == 1 and b"null pointer" in lib.vqa_last_error()    # prob
    assert f(None, 12, 3, 12, 2, 16, 16, None, None) == 1 and b"null pointer" in lib.vqa_last_error()  # logits
    assert f(16, 12, 0, 12, 2, 16, 16, None, None) == 0                                                # B = 0: no launch
    assert f(16, 12, 0, 12, 13, 16, 16, None, None) == 1                                               # ... but k is checked


def test_public_names():
    import dl_vqa_amd
    from dl_vqa_amd import TopAnswers, topk_answers
    assert "TopAnswers" in dl_vqa_amd.__all__ and "topk_answers" in dl_vqa_amd.__all__
    assert TopAnswers._fields == ("indices", "probs") and issubclass(TopAnswers, tuple)
    doc = topk_answers.__doc__
    assert "smaller column" in doc and "a_idx - 1" in doc


@pytest.mark.parametrize("k", [0, -1, 13, 65])
def test_topk_answers_rejects_k_before_the_device_check(k):
    from dl_vqa_amd import topk_answers
    with pytest.raises(ValueError, match="k="):
        topk_answers(torch.zeros(3, 12), k)                       # a CPU tensor: k is judged first
    with pytest.raises(ValueError, match="k="):
        topk_answers(torch.zeros(3, 3000), 65)


def test_topk_answers_rejects_shape_and_cpu_tensors():
    from dl_vqa_amd import topk_answers
    for bad in (torch.zeros(12), torch.zeros(2, 3, 12), torch.zeros(())):
        with pytest.raises(ValueError, match="expected"):
            topk_answers(bad, 1)
    with pytest.raises(ValueError, match="int"):
        topk_answers(torch.zeros(3, 12), 1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        topk_answers(torch.zeros(3, 12), 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        topk_answers(torch.zeros(3, 12, dtype=torch.float64))     # k = 1 by default


def test_predict_validates_k_first_then_raises_what_answer_raises():
    from dl_vqa_amd import VqaNet
    g = Golden("tiny_plus")
    m = VqaNet(tiny_cfg(g.meta), g.meta["V"])                     # A = 12, train mode, on the CPU
    m.load_state_dict(g.sd)
    q, ql = g.t["q"], g.t["q_len"]
    for k in (0, 13, 65):
        with pytest.raises(ValueError, match="k="):
            m.predict(None, q, ql, [0, 1, 2], k=k)                # before the training-mode check
    with pytest.raises(RuntimeError, match="training mode"):
        m.predict(None, q, ql, [0, 1, 2], k=3)
    m.eval()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.predict(None, q, ql, [0, 1, 2], k=3)                    # eval mode on the CPU: answer()'s device check speaks
    with pytest.raises(ValueError, match="k="):
        m.eval().predict(None, q, ql, [0, 1, 2], k=0)
    assert m._last_ctx is None
    mb = VqaNet(full_cfg(16), 30, compute_dtype="bf16")
    with pytest.raises(NotImplementedError, match="compute_dtype"):
        mb.predict(None, q, ql, [0, 1, 2])
