"""CPU: the reference the top-k tests compare against (tests/topk_ref.py) is pinned by itself -- against torch.topk where
torch.topk is specified (pairwise distinct entries), and against hand-written expectations where it is not (ties, signed
zeros, NaN)."""
import math

import torch

from tests.topk_ref import sort_key, topk_reference


def test_reference_equals_torch_topk_on_distinct_rows():
    g = torch.Generator().manual_seed(3)
    for B, A, k in [(4, 12, 12), (3, 257, 32), (5, 1000, 5), (2, 3000, 10), (1, 1, 1)]:
        x = torch.randn(B, A, generator=g) * 3
        assert all(x[b].unique().numel() == A for b in range(B))
        idx, prob, lse = topk_reference(x, k)
        val, want = torch.topk(x, k, dim=1)
        assert idx.dtype == torch.int64 and torch.equal(idx, want)
        assert torch.equal(torch.gather(x, 1, idx), val)
        sm = torch.softmax(x.double(), dim=1)
        assert torch.allclose(prob, torch.gather(sm, 1, idx), rtol=1e-12, atol=0)
        assert torch.allclose(lse, torch.logsumexp(x.double(), 1), rtol=1e-14, atol=0)
        assert bool((prob[:, :-1] >= prob[:, 1:]).all())


def test_reference_on_ties_and_signed_zeros_by_hand():
    x = torch.tensor([[1.0, 3.0, 3.0, -0.0, 0.0, 3.0]])
    idx, prob, _ = topk_reference(x, 6)
    assert idx.tolist() == [[1, 2, 5, 0, 3, 4]]              # the 3s by column, then 1, then -0.0 before +0.0: by column
    den = 3 * math.exp(3) + math.exp(1) + 2
    want = [math.exp(3) / den] * 3 + [math.exp(1) / den] + [1 / den] * 2
    assert torch.allclose(prob, torch.tensor([want], dtype=torch.float64), rtol=1e-14, atol=0)
    # +0.0 in front of -0.0 in the row: still by column, not by sign
    assert topk_reference(torch.tensor([[0.0, -1.0, -0.0]]), 2)[0].tolist() == [[0, 2]]
    # all equal: 0, 1, 2, ...
    assert topk_reference(torch.zeros(2, 9), 4)[0].tolist() == [[0, 1, 2, 3]] * 2
    # the first column is the arg-max torch.max reports (the first maximum)
    t = torch.tensor([[2.0, 5.0, 5.0, 1.0], [7.0, 7.0, 7.0, 7.0]])
    assert topk_reference(t, 1)[0][:, 0].tolist() == t.max(dim=1).indices.tolist() == [1, 0]


def test_reference_on_nan_and_inf_rows():
    nan, inf = float("nan"), float("inf")
    x = torch.tensor([[0.5, nan, inf, -1.0, nan, 2.0],
                      [0.5, 0.25, 4.0, -1.0, 0.0, 2.0]])
    idx, prob, lse = topk_reference(x, 4)
    assert idx.tolist() == [[1, 4, 2, 5], [2, 5, 0, 1]]      # NaNs first, by column, then +inf, then the finite values
    assert bool(torch.isnan(prob[0]).all()) and math.isnan(float(lse[0]))
    assert bool(torch.isfinite(prob[1]).all()) and abs(float(torch.softmax(x[1].double(), 0)[2]) - float(prob[1, 0])) < 1e-15
    key = sort_key(x)
    assert key[0].tolist()[1] == inf and key[0].tolist()[2] == 1e300 and float(key[0, 0]) == 0.5
    # -inf sorts last and takes probability 0
    y = torch.tensor([[-inf, 1.0, -inf, 0.0]])
    idx, prob, _ = topk_reference(y, 4)
    assert idx.tolist() == [[1, 3, 0, 2]] and prob[0, 2:].tolist() == [0.0, 0.0]
