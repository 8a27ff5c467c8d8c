"""CPU: what only VqaNet.explain_shapley / explain_shapley_pairs refuse before any device work: the permutations, seed and
orders arguments.  What the whole explain family refuses is in tests/test_explain_refusals_cpu.py, these two calls included."""
import pytest
import torch

from dl_vqa_amd import shapley_orders
from tests.explain_util import host_caches, invoke, tiny

# name, pairs form, the extra arguments of the device-check calls, those of the call in which the host finds nothing wrong
CALLS = [("explain_shapley", False, dict(permutations=2), dict(permutations=256, seed=5)),
         ("explain_shapley_pairs", True, dict(answers=[0, 1, 2], orders=[[3, 1, 0, 2]]), dict(orders=shapley_orders(256, 4, 1)))]
IDS = [call[0] for call in CALLS]


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
