"""CPU: cached question features (VqaNet.encode_questions / answer_pairs / predict_pairs, dl_vqa_amd.unique_questions) -- the
host-side deduplication, the order of the errors the public calls raise before any device work, the two new entry points
in the header, the ctypes prototypes and the built library, and their host-side argument validation."""
import re

import pytest
import torch

from dl_vqa_amd import ImageFeatures, QuestionFeatures, VqaNet, unique_questions
from tests.golden_util import Golden, full_cfg, tiny_cfg

NEW_ENTRY_POINTS = ("vqa_att_score_grouped_pairs_fwd", "vqa_gather_rows")


# ----------------------------------------------------------------------------- unique_questions
def _masked(q, ql):
    return q * (torch.arange(q.shape[1])[None, :] < ql[:, None])


def test_unique_questions_first_occurrence_order_and_tails():
    q = torch.tensor([[5, 6, 7, 9],      # length 2: the tail 7, 9 is never read
                      [1, 2, 0, 0],
                      [5, 6, 3, 3],      # the same question as row 0 behind another tail
                      [1, 2, 3, 0],      # longer than row 1
                      [5, 6, 7, 9],      # row 0's tokens at full length: another question
                      [1, 2, 8, 8]])     # row 1 again
    ql = torch.tensor([2, 2, 2, 3, 4, 2])
    qu, qlu, qi = unique_questions(q, ql)
    assert qi.dtype == torch.int64 and not qu.is_cuda
    assert qi.tolist() == [0, 1, 0, 2, 3, 1]                       # numbered by first occurrence
    assert qu.tolist() == [[5, 6, 0, 0], [1, 2, 0, 0], [1, 2, 3, 0], [5, 6, 7, 9]]      # tails zeroed
    assert qlu.tolist() == [2, 2, 3, 4]
    assert torch.equal(qu[qi], _masked(q, ql)) and torch.equal(qlu[qi], ql)
    # lists and other integer dtypes work too
    qu2, qlu2, qi2 = unique_questions(q.to(torch.int32).tolist(), ql.tolist())
    assert torch.equal(qu2, qu) and torch.equal(qlu2, qlu) and torch.equal(qi2, qi)


def test_unique_questions_same_tokens_other_length_are_distinct():
    # token 0 inside the length is a token, not padding: [4, 0] at length 2 is not [4] at length 1
    qu, qlu, qi = unique_questions(torch.tensor([[4, 0], [4, 0]]), torch.tensor([1, 2]))
    assert qi.tolist() == [0, 1] and qlu.tolist() == [1, 2] and qu.tolist() == [[4, 0], [4, 0]]


def test_unique_questions_no_repeats_all_equal_and_empty():
    g = torch.Generator().manual_seed(3)
    q = torch.randint(1, 50, (40, 6), generator=g)
    q[:, 0] = torch.randperm(40, generator=g) + 100                # every row distinct, in no sorted order
    ql = torch.randint(1, 7, (40,), generator=g)
    qu, qlu, qi = unique_questions(q, ql)
    assert qu.shape == (40, 6) and qi.tolist() == list(range(40))  # M == B, first-occurrence order is the input order
    assert torch.equal(qu, _masked(q, ql)) and torch.equal(qlu, ql)
    same = torch.tensor([[7, 8, 1], [7, 8, 2], [7, 8, 3]])
    qu, qlu, qi = unique_questions(same, torch.tensor([2, 2, 2]))
    assert qu.tolist() == [[7, 8, 0]] and qlu.tolist() == [2] and qi.tolist() == [0, 0, 0]      # M == 1
    qu, qlu, qi = unique_questions(torch.zeros(0, 5, dtype=torch.int64), torch.zeros(0, dtype=torch.int64))
    assert qu.shape == (0, 5) and qlu.shape == (0,) and qi.shape == (0,)


def test_unique_questions_is_deterministic_under_permutation_of_later_rows():
    g = torch.Generator().manual_seed(5)
    base = torch.randint(1, 9, (6, 4), generator=g)
    bl = torch.randint(1, 5, (6,), generator=g)
    pick = torch.randint(0, 6, (50,), generator=g)
    q, ql = base[pick], bl[pick]
    qu, qlu, qi = unique_questions(q, ql)
    seen = []
    for b in range(50):
        key = (int(ql[b]), tuple(_masked(q, ql)[b].tolist()))
        if key not in seen:
            seen.append(key)
        assert qi[b] == seen.index(key)
    assert [(int(n), tuple(r.tolist())) for r, n in zip(qu, qlu)] == seen


def test_unique_questions_length_errors():
    q = torch.ones(3, 4, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="at least 1"):
        unique_questions(q, torch.tensor([1, 0, 2]))
    with pytest.raises(RuntimeError, match="exceeds the padded question width"):
        unique_questions(q, torch.tensor([1, 5, 2]))
    with pytest.raises(ValueError, match="expected"):
        unique_questions(q, torch.tensor([1, 2]))


# ----------------------------------------------------------------------------- error order without a device
def _tiny():
    g = Golden("tiny_plus")
    m = VqaNet(tiny_cfg(g.meta), g.meta["V"])
    m.load_state_dict(g.sd)
    return g, m


def _host_caches(m, N=3, M=2):
    """Holders as encode_images / encode_questions build them, around host tensors (nothing here reaches a device; the
    model's flat buffer is stood in for by one host tensor so that the ownership marks can be taken)."""
    eng = m._engine
    m._flat_param = torch.zeros(4)
    feats = ImageFeatures(torch.zeros(N, 4, eng.C), torch.zeros(N * 4, eng.mid), (2, 2), m)
    qfeats = QuestionFeatures(torch.zeros(M, eng.Q), torch.zeros(M, eng.mid), m)
    assert feats.N == N and qfeats.M == M
    return feats, qfeats


def test_bf16_then_train_mode_then_device():
    m = VqaNet(full_cfg(16), 30, compute_dtype="bf16")              # train mode, on the CPU
    q, ql = torch.ones(1, 3, dtype=torch.int64), torch.tensor([3])
    for call in (lambda: m.encode_questions(q, ql), lambda: m.answer_pairs(None, None, [0], [0]),
                 lambda: m.predict_pairs(None, None, [0], [0], k=1)):
        with pytest.raises(NotImplementedError, match="compute_dtype"):
            call()
    m.eval()
    with pytest.raises(NotImplementedError, match="compute_dtype"):
        m.encode_questions(q, ql)

    g, m = _tiny()
    m.train()
    for call in (lambda: m.encode_questions(g.t["q"], g.t["q_len"]), lambda: m.answer_pairs(None, None, [0], [0]),
                 lambda: m.predict_pairs(None, None, [0], [0], k=1)):
        with pytest.raises(RuntimeError, match="training mode"):
            call()
    m.eval()                                                        # eval mode on the CPU: the device check speaks
    with pytest.raises(RuntimeError, match="cuda"):
        m.encode_questions(g.t["q"], g.t["q_len"])
    assert m._last_ctx is None and m._flat_param is None


def test_predict_pairs_judges_k_first():
    g, m = _tiny()                                                  # train mode: k is still judged before it
    for k in (0, 13, 65, 1.0, True):
        with pytest.raises(ValueError, match="k"):
            m.predict_pairs(None, None, [0], [0], k=k)
    with pytest.raises(RuntimeError, match="training mode"):
        m.predict_pairs(None, None, [0], [0], k=2)


def test_foreign_objects_index_length_and_range_before_any_device_work():
    g, m = _tiny()
    m.eval()
    feats, qfeats = _host_caches(m, N=3, M=2)
    with pytest.raises(TypeError, match="encode_images"):
        m.answer_pairs(torch.zeros(3), qfeats, [0], [0])
    with pytest.raises(TypeError, match="encode_questions"):
        m.answer_pairs(feats, feats, [0], [0])
    with pytest.raises(TypeError, match="encode_questions"):
        m.predict_pairs(feats, (qfeats.qf, qfeats.qprime), [0], [0])
    with pytest.raises(ValueError, match="3 image_index entries for 2 question_index"):
        m.answer_pairs(feats, qfeats, [0, 1, 2], [0, 1])
    with pytest.raises(IndexError, match=r"image_index entry 3 out of range \[0, 3\)"):
        m.answer_pairs(feats, qfeats, [0, 3], [0, 1])
    with pytest.raises(IndexError, match=r"image_index entry -1"):
        m.answer_pairs(feats, qfeats, torch.tensor([-1, 0]), [0, 1])
    with pytest.raises(IndexError, match=r"question_index entry 2 out of range \[0, 2\)"):
        m.answer_pairs(feats, qfeats, [0, 1], torch.tensor([1, 2], dtype=torch.int32))
    with pytest.raises(IndexError, match=r"question_index entry -1"):
        m.answer_pairs(feats, qfeats, [0, 1], [-1, 0])
    # everything the host can judge is in order: now the device check speaks (the model is on the CPU)
    with pytest.raises(RuntimeError, match="cuda"):
        m.answer_pairs(feats, qfeats, [0, 1, 2, 2], [1, 0, 1, 1])
    assert m._last_ctx is None


# ----------------------------------------------------------------------------- ABI
def test_new_entry_points_in_header_prototypes_and_library():
    from dl_vqa_amd import _lib, build
    build.build_library(verbose=False)
    with open(_lib.HEADER_PATH) as f:
        header = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    assert _lib.header_abi_version() == 9
    for name in NEW_ENTRY_POINTS:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in _lib.PROTOTYPES, name
    lib = _lib.load()
    assert lib.vqa_abi_version() == 9
    for name in NEW_ENTRY_POINTS:
        assert hasattr(lib, name), name


def test_pairs_score_argument_validation_without_gpu():
    """Every check runs on the host before any HIP call.  Arguments: vprime, qp, qrow, wx, wx_ld, bx, order, offsets, score,
    N, B, M, P, mid, G, mode, stream (pointers are made-up 16-byte-aligned integers: nothing dereferences them)."""
    from dl_vqa_amd import _lib
    lib = _lib.load()
    f = lib.vqa_att_score_grouped_pairs_fwd
    assert f(16, 16, 16, 16, 8, 16, 16, 16, 16, 2, 3, 2, 4, 8, 9, 0, None) == 1 and b"glimpses" in lib.vqa_last_error()
    assert f(16, 16, 16, 16, 8, 16, 16, 16, 16, 2, 3, 2, 4, 6, 2, 0, None) == 1 and b"mid=6" in lib.vqa_last_error()
    assert f(16, 16, None, 16, 8, 16, 16, 16, 16, 2, 3, 2, 4, 8, 2, 0, None) == 1 and b"null qrow" in lib.vqa_last_error()
    assert f(16, 16, 16, 16, 8, 16, None, 16, 16, 2, 3, 2, 4, 8, 2, 0, None) == 1 and b"order" in lib.vqa_last_error()
    assert f(16, 16, 16, 16, 8, 16, 16, 16, 16, 2, 3, 0, 4, 8, 2, 0, None) == 1 and b"M=0" in lib.vqa_last_error()
    assert f(16, 16, 16, 16, 8, 16, 16, 16, 16, 2, 3, 2, 4, 8, 2, 3, None) == 1 and b"mode 3" in lib.vqa_last_error()
    assert f(16, 20, 16, 16, 8, 16, 16, 16, 16, 2, 3, 2, 4, 8, 2, 0, None) == 1 and b"aligned" in lib.vqa_last_error()
    assert f(16, 16, 16, 16, 8, 16, 16, 16, 16, 2, 0, 2, 4, 8, 2, 0, None) == 0                       # B = 0: no launch


def test_gather_rows_argument_validation_without_gpu():
    """src, src_ld, rows, dst, dst_ld, B, M, cols, stream."""
    from dl_vqa_amd import _lib
    lib = _lib.load()
    f = lib.vqa_gather_rows
    assert f(16, 8, None, 16, 8, 2, 3, 8, None) == 1 and b"null pointer" in lib.vqa_last_error()
    assert f(16, 8, 16, 16, 8, 2, 0, 8, None) == 1 and b"out of range" in lib.vqa_last_error()      # M = 0
    assert f(16, 8, 16, 16, 8, 2, 3, 0, None) == 1 and b"out of range" in lib.vqa_last_error()      # cols = 0
    assert f(16, 4, 16, 16, 8, 2, 3, 8, None) == 1 and b"src_ld=4" in lib.vqa_last_error()
    assert f(16, 8, 16, 16, 7, 2, 3, 8, None) == 1 and b"dst_ld=7" in lib.vqa_last_error()
    assert f(16, 8, 16, 16, 8, 0, 3, 8, None) == 0                                                  # B = 0: no launch
