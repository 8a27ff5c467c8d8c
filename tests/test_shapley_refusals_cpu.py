"""CPU: what VqaNet.explain_shapley / explain_shapley_pairs refuse before any device work, in the pattern of
tests/test_explain_refusals_cpu.py: bf16, train mode and the device check in that order; the permutations, seed and orders
arguments; the type of feats and qfeats, a bank without v', the index count and the `answers` argument."""
import pytest
import torch

from dl_vqa_amd import VqaNet, shapley_orders
from tests.explain_util import host_caches, tiny
from tests.golden_util import full_cfg
from tests.test_explain_refusals_cpu import invoke

# name, pairs form, the extra arguments of the device-check calls, those of the call in which the host finds nothing wrong
CALLS = [("explain_shapley", False, dict(permutations=2), dict(permutations=256, seed=5)),
         ("explain_shapley_pairs", True, dict(answers=[0, 1, 2], orders=[[3, 1, 0, 2]]), dict(orders=shapley_orders(256, 4, 1)))]
IDS = [call[0] for call in CALLS]


@pytest.mark.parametrize("name,pairs,device_kw,extra", CALLS, ids=IDS)
def test_bf16_then_train_mode_then_device(name, pairs, device_kw, extra):
    m = VqaNet(full_cfg(16), 30, compute_dtype="bf16")              # train mode, on the CPU
    q, ql = torch.ones(1, 3, dtype=torch.int64), torch.tensor([3])
    with pytest.raises(NotImplementedError, match="compute_dtype"):  # before permutations is looked at
        getattr(m, name)(None, None, [0], [0], permutations=3) if pairs else getattr(m, name)(None, q, ql, [0], permutations=3)
    g, m = tiny()
    m.train()
    with pytest.raises(RuntimeError, match="training mode"):
        getattr(m, name)(None, None, [0], [0], permutations=3) if pairs else \
            getattr(m, name)(None, g.t["q"], g.t["q_len"], [0, 1, 2], permutations=3)
    m.eval()                                                        # eval mode on the CPU: the device check speaks
    feats, qfeats = host_caches(m)
    with pytest.raises(RuntimeError, match="cuda"):
        invoke(m, name, pairs, feats, qfeats, g.t["q"][:3], g.t["q_len"][:3], [0, 1, 2], **device_kw)
    assert m._last_ctx is None


@pytest.mark.parametrize("name,pairs,device_kw,extra", CALLS, ids=IDS)
def test_permutations_seed_and_orders_are_judged_on_the_host(name, pairs, device_kw, extra):
    g, m = tiny()
    m.eval()
    feats, qfeats = host_caches(m, N=3, M=2)                        # a 2 x 2 grid: P = 4
    q, ql = g.t["q"][:3], g.t["q_len"][:3]
    call = lambda **kw: invoke(m, name, pairs, feats, qfeats, q, ql, [0, 1, 2], **kw)
    rng = torch.get_rng_state()
    for bad in (True, 4.0, "4", None, torch.tensor(4)):
        with pytest.raises(TypeError, match=f"VqaNet.{name}: permutations must be an int"):
            call(permutations=bad)
    for bad in (0, 1, 3, 15, 258, -2, 1024):
        with pytest.raises(ValueError, match=f"VqaNet.{name}: permutations must be an even int in 2..256"):
            call(permutations=bad)
    for bad in (True, 1.5, "0"):
        with pytest.raises(TypeError, match=f"VqaNet.{name}: seed must be an int"):
            call(seed=bad)
    # orders: an integer tensor [M, 4], 1 <= M <= 128, every row a permutation
    for bad in (torch.zeros(2, 4), torch.zeros(2, 4, dtype=torch.bool), [[0.0, 1.0, 2.0, 3.0]]):
        with pytest.raises(TypeError, match=f"VqaNet.{name}: orders must be an integer tensor"):
            call(orders=bad)
    for bad in (torch.arange(4), torch.zeros(0, 4, dtype=torch.int64), torch.arange(4).expand(129, 4),
                torch.arange(4).view(1, 1, 4)):
        with pytest.raises(ValueError, match=rf"VqaNet.{name}: orders of shape .* \(expected \[M, P\] with 1 <= M <= 128\)"):
            call(orders=bad)
    for bad in (torch.arange(5)[None], torch.arange(3)[None]):
        with pytest.raises(ValueError, match=rf"VqaNet.{name}: orders of shape .* on a 2 x 2 grid \(expected \[M, 4\]\)"):
            call(orders=bad)
    for bad, row in (([[0, 1, 2, 3], [0, 1, 1, 3]], 1), ([[0, 1, 2, 4]], 0), ([[3, 2, 1, 0], [1, 2, 3, 0], [-1, 0, 1, 2]], 2)):
        with pytest.raises(ValueError, match=rf"VqaNet.{name}: orders row {row} is no permutation of 0\.\.3"):
            call(orders=bad)
    # orders replaces permutations / seed: those are not looked at
    with pytest.raises(RuntimeError, match="cuda"):
        call(orders=[[0, 1, 2, 3]], permutations=3, seed=None)
    with pytest.raises(RuntimeError, match="cuda"):
        call(orders=torch.tensor([[2, 0, 3, 1]], dtype=torch.int32))
    # the argument's own check comes before the features are looked at, as the window of explain_occlusion
    with pytest.raises(ValueError, match="permutations must be an even int"):
        getattr(m, name)(torch.zeros(3), qfeats, [0], [0], permutations=3) if pairs else \
            getattr(m, name)(torch.zeros(3), q, ql, [0, 1, 2], permutations=3)
    assert torch.equal(torch.get_rng_state(), rng) and m._last_ctx is None


@pytest.mark.parametrize("name,pairs,device_kw,extra", CALLS, ids=IDS)
def test_features_index_and_answers_are_judged_before_any_device_work(name, pairs, device_kw, extra):
    g, m = tiny()
    m.eval()
    A = m._engine.A
    feats, qfeats = host_caches(m, N=3, M=2)
    q, ql = g.t["q"][:3], g.t["q_len"][:3]
    call = lambda index=(0, 1, 2), **kw: invoke(m, name, pairs, feats, qfeats, q, ql, list(index), **kw)
    with pytest.raises(TypeError, match="encode_images"):
        getattr(m, name)(torch.zeros(3), qfeats, [0], [0]) if pairs else getattr(m, name)(torch.zeros(3), q, ql, [0, 1, 2])
    if pairs:
        with pytest.raises(TypeError, match="encode_questions"):
            getattr(m, name)(feats, feats, [0], [0])
    with pytest.raises(ValueError, match="2 answers for 3"):
        call(answers=[0, 1])
    with pytest.raises(IndexError, match=rf"answers entry {A} out of range \[0, {A}\)"):
        call(answers=[0, A, 1])
    with pytest.raises(IndexError, match="answers entry -1"):
        call(answers=torch.tensor([0, 1, -1], dtype=torch.int32))
    with pytest.raises(TypeError, match="integer"):
        call(answers=[0.0, 1.0, 2.0])
    m._ensure_flat = lambda: None                                   # as on a device: the index and ownership checks speak
    with pytest.raises(ValueError, match="2 image_index entries for 3"):
        call(index=(0, 1))
    with pytest.raises(IndexError):
        call(index=(0, 1, 3))
    _, other = tiny()
    with pytest.raises(RuntimeError, match="belong elsewhere"):
        invoke(m, name, pairs, host_caches(other)[0], qfeats, q, ql, [0, 1, 2])
    bank, qfeats = host_caches(m, vprime=False)                     # a bank without v' (the caches above are stale now)
    with pytest.raises(RuntimeError, match="with_vprime=False"):
        invoke(m, name, pairs, bank, qfeats, q, ql, [0, 1, 2])
    del m._ensure_flat
    feats, qfeats = host_caches(m, N=3, M=2)
    with pytest.raises(RuntimeError, match="cuda"):                 # everything the host can judge is in order
        call(answers=[0, A - 1, 1], **extra)
    assert m._last_ctx is None and all(p.grad is None for p in m.parameters())
