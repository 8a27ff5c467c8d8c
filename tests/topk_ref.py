"""Reference for vqa_softmax_topk / topk_answers / VqaNet.predict (include/vqa_hip.h): a STABLE descending sort of the row.

The total order: larger value first; equal values by smaller column; -0.0 equals +0.0; NaN ranks above +inf, several NaNs
by column.  torch.sort(descending=True, stable=True) is that order once -0.0 is canonicalised and NaN is sent in front,
which is done here by sorting a float64 copy in which NaN is replaced by +inf and every +inf already there is kept below
it (finite fp32 values and +-inf are exact in float64, and fp32's largest finite value is far below float64's).
The probabilities are a float64 softmax of the row, gathered at the picks; a row that holds a NaN gets NaN."""
import torch


def sort_key(x: torch.Tensor) -> torch.Tensor:
    """float64 [B, A]: the same order as x under a plain descending comparison: -0.0 -> +0.0, +inf -> 1e300, NaN -> +inf."""
    x = x.detach().cpu()
    assert x.dtype == torch.float32 and x.dim() == 2
    key = x.double() + 0.0                                   # -0.0 + 0.0 = +0.0
    key = torch.where(torch.isposinf(key), torch.full_like(key, 1e300), key)
    return torch.where(torch.isnan(key), torch.full_like(key, float("inf")), key)


def topk_reference(x: torch.Tensor, k: int):
    """x fp32 [B, A] -> (idx int64 [B, k], prob float64 [B, k], lse float64 [B])."""
    x = x.detach().cpu()
    _, order = torch.sort(sort_key(x), dim=1, descending=True, stable=True)
    idx = order[:, :k].contiguous()
    xd = x.double()
    lse = torch.logsumexp(xd, dim=1)                         # NaN rows: NaN
    prob = torch.exp(torch.gather(xd, 1, idx) - lse[:, None])
    nan_row = torch.isnan(xd).any(dim=1)
    prob[nan_row] = float("nan")
    lse[nan_row] = float("nan")
    return idx, prob, lse
