"""Drop-in ``VqaNet`` whose forward/backward run on the HIP kernel library.

Mirrors the reference's module interface (models/model.py:7-67): same constructor
``VqaNet(cfg, embedding_tokens)``, same ``forward(v, q, q_len) -> [B, max_answers]``, same
sub-module attribute names (``text``, ``image``, ``attention``, ``classifier`` — read by
utils/main_utils.py:21-41) and the same ``state_dict`` keys/shapes, so ``model.pth`` checkpoints
interchange (utils/train_logger.py:95-112, evaluate_vqa.py:72-75).

The sub-modules are parameter containers built from the same torch constructors in the same order
as the reference, so ``torch.manual_seed(s); VqaNet(cfg, V)`` yields bit-identical initial
weights.  Their parameters live in ONE flat fp32 buffer (ordered as backward produces the
gradients) so that the optimiser and the data-parallel all-reduce work on contiguous ranges.
"""
from __future__ import annotations

import warnings
import weakref
from collections import OrderedDict
from functools import partial
from types import SimpleNamespace
from typing import Dict, List, NamedTuple, Optional

import torch
import torch.nn as nn

from . import ops
from .engine import Engine


class questionNet(nn.Module):
    """Parameter container for models/model.py:134-166 (Embedding pad 0 -> Dropout -> Tanh -> LSTM -> c_n)."""

    def __init__(self, embedding_tokens, embedding_features, lstm_features, num_lstm_layers, drop, bidirectional):
        super().__init__()
        self.embedding = nn.Embedding(num_embeddings=embedding_tokens, embedding_dim=embedding_features, padding_idx=0)
        self.drop = nn.Dropout(drop)
        self.tanh = nn.Tanh()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")   # torch warns that dropout is a no-op with one layer (as in the reference)
            self.lstm = nn.LSTM(input_size=embedding_features, hidden_size=lstm_features, num_layers=num_lstm_layers,
                                dropout=drop, bidirectional=bidirectional)


class ImageNet2(nn.Sequential):
    """Parameter container for models/model.py:72-84 ([Conv2d k3, ReLU, MaxPool2d(2,2)] x n + Dropout)."""

    def __init__(self, image_cfg):
        super().__init__()
        ch = image_cfg["num_channels"]
        for i in range(len(ch) - 1):
            self.add_module(f"conv{i}", nn.Conv2d(ch[i], ch[i + 1], kernel_size=image_cfg["kernel_size"],
                                                  stride=image_cfg["stride"]))
            self.add_module(f"relu{i}", nn.ReLU())
            self.add_module(f"maxpool{i}", nn.MaxPool2d(2, 2))
        self.add_module("drop", nn.Dropout(image_cfg["dropout"]))


class Attention(nn.Module):
    """Parameter container for models/model.py:169-195."""

    def __init__(self, v_features, q_features, mid_features, glimpses, do_option, drop=0.0):
        super().__init__()
        self.do_option = do_option
        self.v_conv = nn.Conv2d(v_features, mid_features, kernel_size=1, bias=False)
        self.q_lin = nn.Linear(q_features, mid_features)
        self.x_conv = nn.Conv2d(2 * mid_features if do_option == "|" else mid_features, glimpses, kernel_size=1)
        self.drop = nn.Dropout(drop)
        self.relu = nn.ReLU(inplace=True)


class Classifier(nn.Sequential):
    """Parameter container for models/model.py:198-205."""

    def __init__(self, in_features, mid_features, out_features, drop=0.0):
        super().__init__()
        self.add_module("drop1", nn.Dropout(drop))
        self.add_module("lin1", nn.Linear(in_features, mid_features))
        self.add_module("relu", nn.ReLU())
        self.add_module("drop2", nn.Dropout(drop))
        self.add_module("lin2", nn.Linear(mid_features, out_features))


def _flat_order(names: List[str]) -> List[str]:
    """Parameter order inside the flat buffer = the order backward produces gradients."""
    def key(n):
        if n.startswith("classifier."):
            return (0, 0 if "lin2" in n else 1, n)
        if n.startswith("attention."):
            return (1, 0, n)
        if n.startswith("text.lstm"):
            return (2, 0, n)
        if n.startswith("text."):
            return (2, 1, n)
        if n.startswith("image.conv"):
            return (3, -int(n.split(".")[1][4:]), n)
        return (4, 0, n)
    return sorted(names, key=key)


def validate_question_lengths(q_len, T: int) -> None:
    """pack_padded_sequence (models/model.py:159-162) raises for a length below 1 or above the padded width.  Lengths that
    arrive on the host (the data loader's, before run_batch uploads them) are checked there; device-resident lengths are
    taken as they are -- the recurrence kernels then treat a sample as finished from step q_len[b] on (0: c_n = 0)."""
    if q_len.is_cuda or q_len.numel() == 0:
        return
    lo, hi = int(q_len.min()), int(q_len.max())
    if lo < 1:
        raise RuntimeError(f"question length {lo}: every sample needs a length of at least 1 "
                           "(pack_padded_sequence would raise: models/model.py:159-162)")
    if hi > T:
        raise RuntimeError(f"question length {hi} exceeds the padded question width {T} "
                           "(pack_padded_sequence would raise: models/model.py:159-162)")


def _host_image_index(index, rows: int, what: str = "image_index", of: str = "") -> torch.Tensor:
    """An index into `rows` rows (image_index, or answer_pairs' question_index into `of`) on the host as int64 [B];
    IndexError for an entry outside [0, rows).  The one place where a CUDA index is copied to the host, which synchronises:
    an entry point converts once and hands the result on -- a host int64 tensor passes through as it is."""
    idx = torch.as_tensor(index).detach().to(device="cpu", dtype=torch.int64).reshape(-1)
    if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= rows):
        bad = int(idx.min()) if int(idx.min()) < 0 else int(idx.max())
        raise IndexError(f"{what} entry {bad} out of range [0, {rows})" + (f" ({rows} encoded {of})" if of else ""))
    return idx


def _upload_index(dev, *parts):
    """The host index tensors `parts` on the device `dev` as int32: views of ONE tensor, uploaded in a single copy."""
    return torch.split(torch.cat([p.to(torch.int32) for p in parts]).to(dev), [p.numel() for p in parts])


def _upload_with_columns(dev, index, cols):
    """_upload_index of the host index tensors `index`, together with the answer columns `cols` of explain / explain_pairs
    where those are host data (the same single copy); CUDA columns become int32 on `dev`, None stays None.  Returns (the
    device index tensors, the device columns or None)."""
    if cols is None or cols.is_cuda:
        return _upload_index(dev, *index), (cols if cols is None else cols.to(device=dev, dtype=torch.int32))
    *index, cols = _upload_index(dev, *index, cols)
    return tuple(index), cols


def group_by_image(image_index, N: int):
    """Group questions by the image they ask about: image_index[b] in [0, N) -> (order int32 [B], offsets int32 [N+1]) on
    the host; the questions of image n are order[offsets[n]:offsets[n+1]], in their original order (a stable counting
    sort).  IndexError for an entry outside [0, N).  An index that is on the host as int64 already is used as it is."""
    return _group(_host_image_index(image_index, N), N)


def _group(idx, N: int):
    """group_by_image of an index that _host_image_index has converted and checked: the VqaNet entry points convert theirs
    once and group that tensor."""
    offsets = torch.zeros(N + 1, dtype=torch.int64)
    if idx.numel():
        offsets[1:] = torch.cumsum(torch.bincount(idx, minlength=N), 0)
    order = torch.argsort(idx, stable=True)
    return order.to(torch.int32), offsets.to(torch.int32)


def compact_image_index(image_index, N: int):
    """The distinct rows of an N-row feature bank that a batch asks about, and the batch grouped by them: image_index[b] in
    [0, N) -> (rows int32 [n_u], slot int32 [B], order int32 [B], offsets int32 [n_u+1]) on the host.  rows holds the distinct
    entries of image_index, ascending; slot[b] is the position of image_index[b] in rows (rows[slot[b]] == image_index[b]);
    (order, offsets) = group_by_image(slot, n_u).  IndexError for an entry outside [0, N), as group_by_image raises it."""
    idx = _host_image_index(image_index, N)
    rows, slot = torch.unique(idx, sorted=True, return_inverse=True)
    order, offsets = _group(slot, rows.numel())
    return rows.to(torch.int32), slot.to(torch.int32), order, offsets


class TopAnswers(NamedTuple):
    """What topk_answers / VqaNet.predict return: indices int64 [B, k] (0-based answer columns, best first) and probs
    fp32 [B, k] (their softmax probabilities)."""
    indices: torch.Tensor
    probs: torch.Tensor


class Attribution(NamedTuple):
    """What VqaNet.explain / explain_pairs return: maps fp32 [B, gh, gw] -- the gradient x input map R[b, p] of each question
    on the feature grid (signed, no upsampling, no normalisation) --, answers int64 [B] -- the answer column each map explains
    (0-based, as TopAnswers.indices) -- and logits fp32 [B, A] -- what answer() / answer_pairs() return for the same
    arguments, bit for bit."""
    maps: torch.Tensor
    answers: torch.Tensor
    logits: torch.Tensor


class WordAttribution(NamedTuple):
    """What VqaNet.explain_words returns: words fp32 [B, T] -- the gradient x input value of each token slot of each question
    (signed, not normalised; 0 for t >= q_len[b]) -- and explain()'s maps fp32 [B, gh, gw], answers int64 [B] and logits fp32
    [B, A] for the same arguments, bit for bit."""
    words: torch.Tensor
    maps: torch.Tensor
    answers: torch.Tensor
    logits: torch.Tensor


class Occlusion(NamedTuple):
    """What VqaNet.explain_occlusion / explain_occlusion_pairs return: maps fp32 [B, gh, gw] -- how far the explained logit
    falls when the window around each grid position is taken out of the image (signed, no upsampling, no normalisation) --,
    answers int64 [B] -- the answer column each map explains, as Attribution.answers -- and logits fp32 [B, A] -- what answer()
    / answer_pairs() return for the same arguments, bit for bit."""
    maps: torch.Tensor
    answers: torch.Tensor
    logits: torch.Tensor


class WordOcclusion(NamedTuple):
    """What VqaNet.explain_words_occlusion returns: words fp32 [B, T] -- how far the explained logit falls when the embedding
    output of each token slot is replaced by the zero vector (signed, not normalised; +0.0 for t >= q_len[b]) --, answers int64
    [B] -- the answer column each row explains, as Attribution.answers -- and logits fp32 [B, A] -- what answer() returns for the
    same arguments, bit for bit."""
    words: torch.Tensor
    answers: torch.Tensor
    logits: torch.Tensor


class Faithfulness(NamedTuple):
    """What VqaNet.explain_faithfulness / explain_faithfulness_pairs return: deletion fp32 [B, P+1] -- the explained logit with
    the k best-ranked positions of the map absent, k = 0 .. P --, insertion fp32 [B, P+1] -- the same logit with only those k
    positions present --, order int64 [B, P] -- the positions by descending map value, equal values by the smaller position --,
    answers int64 [B] -- the answer column each curve follows, as Attribution.answers -- and logits fp32 [B, A] -- what answer()
    / answer_pairs() return for the same arguments, bit for bit.  A map that ranks well has a deletion curve that falls fast (a
    small deletion_auc) and an insertion curve that rises fast (a large insertion_auc)."""
    deletion: torch.Tensor
    insertion: torch.Tensor
    order: torch.Tensor
    answers: torch.Tensor
    logits: torch.Tensor

    @staticmethod
    def _auc(curve):
        c = curve.double()
        return (c[:, :-1] + c[:, 1:]).sum(1) / (2 * (c.shape[1] - 1))

    def deletion_auc(self):
        """The trapezoid mean of each deletion curve, sum_k (c[k] + c[k+1]) / (2P): float64 [B], formed on the curve's device."""
        return self._auc(self.deletion)

    def insertion_auc(self):
        """The trapezoid mean of each insertion curve, as deletion_auc()."""
        return self._auc(self.insertion)


class ProbabilityCurves(NamedTuple):
    """What VqaNet.explain_faithfulness_probs / explain_faithfulness_probs_pairs return.  With the k best-ranked positions of the
    map absent (deletion) or alone present (insertion), k = 0 .. P: deletion, insertion fp32 [B, P+1] -- the softmax
    probability of the explained column a_b --, deletion_top, insertion_top int32 [B, P+1] -- the arg-max column at that step,
    in topk_answers' order (ties by the smaller column) --, deletion_top_prob, insertion_top_prob fp32 [B, P+1] -- its
    probability --, and Faithfulness' order int64 [B, P], answers int64 [B] and logits fp32 [B, A].  The AUCs are the published
    deletion / insertion metric (on probabilities: adding a constant to every logit does not move them); the flip points say
    how many of the map's best positions must go before the answer changes, and how few suffice to get it back."""
    deletion: torch.Tensor
    insertion: torch.Tensor
    deletion_top: torch.Tensor
    insertion_top: torch.Tensor
    deletion_top_prob: torch.Tensor
    insertion_top_prob: torch.Tensor
    order: torch.Tensor
    answers: torch.Tensor
    logits: torch.Tensor

    def deletion_auc(self):
        """The trapezoid mean of each deletion curve, as Faithfulness.deletion_auc(): float64 [B] on the curve's device."""
        return Faithfulness._auc(self.deletion)

    def insertion_auc(self):
        """The trapezoid mean of each insertion curve, as deletion_auc()."""
        return Faithfulness._auc(self.insertion)

    @staticmethod
    def _first(hit):
        """The smallest k with hit[b, k], P + 1 where there is none: int64 [B] on the device of hit [B, P+1]."""
        steps = torch.arange(hit.shape[1], device=hit.device).expand_as(hit)
        return torch.where(hit, steps, torch.full_like(steps, hit.shape[1])).min(dim=1).values.reshape(hit.shape[0])

    def deletion_flip(self):
        """The smallest k at which the arg-max is no longer the explained column, deletion_top[b, k] != answers[b]: how many
        of the map's best positions must go before the answer changes.  int64 [B] on the device; P + 1 when it never does."""
        return self._first(self.deletion_top != self.answers[:, None])

    def insertion_flip(self):
        """The smallest k at which the arg-max is the explained column, insertion_top[b, k] == answers[b]: how few of the
        map's best positions suffice to get the answer back.  int64 [B] on the device; P + 1 when none does."""
        return self._first(self.insertion_top == self.answers[:, None])


class IntegratedGradients(NamedTuple):
    """What VqaNet.explain_integrated / explain_integrated_pairs return: maps fp32 [B, gh, gw] -- the integrated-gradients map
    of each question on the feature grid, zero baseline, midpoint rule (signed, no upsampling, no normalisation) --, answers
    int64 [B] -- the answer column each map explains, as Attribution.answers --, logits fp32 [B, A] -- what answer() /
    answer_pairs() return for the same arguments, bit for bit -- and baseline_logits fp32 [B] -- the explained logit of each
    question on an image cache of zeros.  The maps sum to logits[b, a_b] - baseline_logits[b] up to the quadrature error:
    completeness_gap() says how far off they are."""
    maps: torch.Tensor
    answers: torch.Tensor
    logits: torch.Tensor
    baseline_logits: torch.Tensor

    def completeness_gap(self):
        """maps.sum over positions - (logits[b, a_b] - baseline_logits[b]): float64 [B], formed on the maps' device.  A column
        outside [0, A) (a zero map, a zero baseline) is read as the nearest column."""
        cols = self.answers.clamp(0, self.logits.shape[1] - 1)[:, None]
        picked = self.logits.gather(1, cols)[:, 0].double()
        return self.maps.double().sum((1, 2)) - (picked - self.baseline_logits.double())


class Shapley(NamedTuple):
    """What VqaNet.explain_shapley / explain_shapley_pairs return: maps fp32 [B, gh, gw] -- the sampled Shapley value of each
    grid position for the explained logit as a function of the set of positions present (signed, no upsampling, no
    normalisation) --, stderr fp32 [B, gh, gw] -- the standard error of each entry over the drawn orders, NaN when one order
    was drawn --, answers int64 [B] -- the answer column each map explains, as Attribution.answers --, logits fp32 [B, A] --
    what answer() / answer_pairs() return for the same arguments, bit for bit -- and baseline_logits fp32 [B] -- the explained
    logit of the empty image, explain_faithfulness()'s insertion[:, 0].  The maps sum to logits[b, a_b] - baseline_logits[b] up
    to fp32 rounding, whatever the orders: completeness_gap() says how far off they are."""
    maps: torch.Tensor
    stderr: torch.Tensor
    answers: torch.Tensor
    logits: torch.Tensor
    baseline_logits: torch.Tensor

    def completeness_gap(self):
        """maps.sum over positions - (logits[b, a_b] - baseline_logits[b]): float64 [B], formed on the maps' device, as
        IntegratedGradients.completeness_gap().  Zero up to fp32 rounding: every order's estimates telescope."""
        return IntegratedGradients.completeness_gap(self)


def shapley_orders(permutations: int, P: int, seed: int = 0) -> torch.Tensor:
    """The table of orders VqaNet.explain_shapley draws for `permutations` permutations (counted with the reverses) of P grid
    positions: int64 [permutations // 2, P] on the host, row m = torch.randperm(P) under ONE CPU torch.Generator seeded with
    `seed`, drawn in ascending m.  The global seed stream is not touched."""
    gen = torch.Generator(device="cpu").manual_seed(int(seed))
    return torch.stack([torch.randperm(P, generator=gen) for _ in range(permutations // 2)]).reshape(permutations // 2, P)


SHAPLEY_MAX_PERMUTATIONS = 256      # explain_shapley: permutations, counted with the reverses; a table holds half as many orders


def _check_permutations(what: str, permutations) -> int:
    """The permutations argument of explain_shapley / explain_shapley_pairs: an even int in 2..256 (a bool is not one)."""
    if isinstance(permutations, bool) or not isinstance(permutations, int):
        raise TypeError(f"{what}: permutations must be an int, got {type(permutations).__name__}")
    if not 2 <= permutations <= SHAPLEY_MAX_PERMUTATIONS or permutations % 2:
        raise ValueError(f"{what}: permutations must be an even int in 2..{SHAPLEY_MAX_PERMUTATIONS} (each drawn order is walked "
                         f"with its reverse), got {permutations}")
    return permutations


def _check_orders(what: str, orders, grid):
    """The orders argument of explain_shapley / explain_shapley_pairs, judged on the host: an integer tensor [M, P], 1 <= M <=
    128, every row a permutation of 0 .. P-1, P = gh * gw.  Returns it on the host as int64; grid None (feats is no
    ImageFeatures, which the next check refuses): the dtype and rank alone."""
    orders = torch.as_tensor(orders).detach()
    if orders.is_floating_point() or orders.is_complex() or orders.dtype == torch.bool:
        raise TypeError(f"{what}: orders must be an integer tensor, got {orders.dtype}")
    if orders.dim() != 2 or not 1 <= orders.shape[0] <= SHAPLEY_MAX_PERMUTATIONS // 2:
        raise ValueError(f"{what}: orders of shape {tuple(orders.shape)} (expected [M, P] with 1 <= M <= "
                         f"{SHAPLEY_MAX_PERMUTATIONS // 2})")
    orders = orders.cpu().long()
    if grid is None:
        return orders
    P = grid[0] * grid[1]
    if orders.shape[1] != P:
        raise ValueError(f"{what}: orders of shape {tuple(orders.shape)} on a {grid[0]} x {grid[1]} grid (expected "
                         f"[M, {P}])")
    if P > (1 << 20):
        raise ValueError(f"{what}: {P} grid positions, the curves take at most {1 << 20}")
    bad = (orders.sort(dim=1).values != torch.arange(P)).any(dim=1).nonzero()
    if bad.numel():
        raise ValueError(f"{what}: orders row {int(bad[0])} is no permutation of 0..{P - 1}")
    return orders


OCCLUSION_WINDOW_MAX = 7    # include/vqa_hip.h vqa_occl_logit
INTEGRATED_MAX_STEPS = 64   # include/vqa_hip.h VQA_ATT_PATH_MAX_STEPS
FAITHFULNESS_MAX_POSITIONS = 8192    # include/vqa_hip.h vqa_rank_desc


def word_occlusion_chunks(lengths, T: int, max_rows: Optional[int] = None):
    """The questions of a batch cut into chunks [(b0, b1), ...] of consecutive questions whose variants -- the pairs (b, t), t <
    min(lengths[b], T), none for a length <= 0 -- number at most max_rows per chunk (None: one chunk).  Chunks cut between
    questions, never inside one: a question with more variants than max_rows is a chunk of its own.  Every question is in
    exactly one chunk, those without variants included.  lengths: host integers."""
    counts = [min(max(int(n), 0), T) for n in lengths]
    if max_rows is None:
        return [(0, len(counts))] if counts else []
    chunks, b0, rows = [], 0, 0
    for b, n in enumerate(counts):
        if b > b0 and rows + n > max_rows:
            chunks.append((b0, b))
            b0, rows = b, 0
        rows += n
    if counts:
        chunks.append((b0, len(counts)))
    return chunks


def word_occlusion_table(lengths, T: int, b0: int = 0, b1: Optional[int] = None):
    """The variant table of VqaNet.explain_words_occlusion for the questions [b0, b1) of a batch of B = len(lengths) questions
    with T token slots, from host lengths.  A variant is a pair (b, t) with t < min(lengths[b], T); there are V of them, none
    for a length <= 0.  Zeroing slot t leaves the forward direction's state before t and the reverse direction's state after t
    unchanged, so a variant's chain starts at time t in both directions.  Per direction the table holds the variant rows in the
    order their chains start and, for every time s, how many have started -- at time s a direction steps its first n[s] rows:

      fwd_b, fwd_t   int32 [V]   ascending t (then b): the chain of row r runs s = t .. ; this is also the row order of the
                                 classifier-input buffer and of the tail
      rev_b, rev_t   int32 [V]   descending t (then ascending b): the chain of row r runs s = t, t - 1, .. 0
      rev_row        int32 [V]   the row of (rev_b[r], rev_t[r]) in the forward order
      fwd_seed       int32 [V]   t * B + b: the row of the base state the forward chain starts from (slot t of [(T+1)*B, H])
      rev_seed       int32 [V]   (t + 1) * B + b: the same for the reverse chain (slot t + 1)
      n_fwd, n_rev   lists [T]   n_fwd[s] = #{t <= s}, n_rev[s] = #{t >= s}
      steps          the chunk's largest clamped length: the loops stop there (n_rev[s] = 0 for s >= steps)
      row_steps      sum over both directions and s < steps of n[s]: the rows of the recurrent products, <= V * (steps + 1)
                     <= V * (T + 1); running every variant in full takes 2 * T * V

    Pure host code: nothing here touches a device."""
    B = len(lengths)
    b1 = B if b1 is None else b1
    counts = torch.as_tensor(lengths, dtype=torch.int64).reshape(-1)[b0:b1].clamp(0, T)
    live = (torch.arange(T)[:, None] < counts[None, :])                     # [T, questions of the chunk], time-major
    fwd = live.nonzero()                                                    # rows (t, i): ascending t, then ascending i
    rev = live.flip(0).nonzero()                                            # rows (T - 1 - t, i): descending t, then ascending i
    fwd_t, fwd_b = fwd[:, 0], fwd[:, 1] + b0
    rev_t, rev_b = T - 1 - rev[:, 0], rev[:, 1] + b0
    V = fwd.shape[0]
    row_of = torch.zeros(T, max(b1 - b0, 1), dtype=torch.int64)
    row_of[fwd[:, 0], fwd[:, 1]] = torch.arange(V)
    per_t = live.sum(1)                                                     # variants whose slot is t
    n_fwd = torch.cumsum(per_t, 0).tolist()
    n_rev = torch.cumsum(per_t.flip(0), 0).flip(0).tolist()
    steps = int(counts.max()) if counts.numel() else 0
    i32 = lambda x: x.to(torch.int32)
    return SimpleNamespace(V=V, b0=b0, b1=b1, steps=steps, n_fwd=n_fwd, n_rev=n_rev,
                           row_steps=sum(n_fwd[:steps]) + sum(n_rev[:steps]),
                           fwd_b=i32(fwd_b), fwd_t=i32(fwd_t), fwd_seed=i32(fwd_t * B + fwd_b),
                           rev_b=i32(rev_b), rev_t=i32(rev_t), rev_seed=i32((rev_t + 1) * B + rev_b),
                           rev_row=i32(row_of[rev_t, rev_b - b0]))


def _check_window(what: str, window) -> int:
    """The window argument of explain_occlusion / explain_occlusion_pairs: an odd int in 1..7 (a bool is not one)."""
    if isinstance(window, bool) or not isinstance(window, int) or not 1 <= window <= OCCLUSION_WINDOW_MAX or window % 2 == 0:
        raise ValueError(f"{what}: window must be an odd int in 1..{OCCLUSION_WINDOW_MAX}, got {window!r}")
    return window


def _check_steps(what: str, steps) -> int:
    """The steps argument of explain_integrated / explain_integrated_pairs: an int in 1..64 (a bool is not one)."""
    if isinstance(steps, bool) or not isinstance(steps, int) or not 1 <= steps <= INTEGRATED_MAX_STEPS:
        raise ValueError(f"{what}: steps must be an int in 1..{INTEGRATED_MAX_STEPS}, got {steps!r}")
    return steps


def integrated_alphas(steps: int) -> torch.Tensor:
    """The step positions of explain_integrated on the host: the midpoint rule alpha_s = float32((2s + 1) / (2 * steps)), s = 0 ..
    steps-1, each rounded once from the double."""
    return torch.tensor([(2 * s + 1) / (2 * steps) for s in range(steps)], dtype=torch.float64).to(torch.float32)


def _check_maps(what: str, maps, B: int, grid):
    """The maps argument of explain_faithfulness / explain_faithfulness_pairs, judged on the host: a floating tensor of B * P
    elements shaped [B, gh, gw] or [B, P], P = gh * gw at most the rank kernel's cap.  grid None (feats is no ImageFeatures,
    which the next check refuses): the dtype alone."""
    if not isinstance(maps, torch.Tensor):
        maps = torch.as_tensor(maps)
    if not maps.is_floating_point():
        raise TypeError(f"{what}: maps must be a floating tensor, got {maps.dtype}")
    if grid is None:
        return
    gh, gw = grid
    P = gh * gw
    if maps.numel() != B * P or tuple(maps.shape) not in ((B, gh, gw), (B, P)):
        raise ValueError(f"{what}: maps of shape {tuple(maps.shape)} for {B} questions on a {gh} x {gw} grid "
                         f"(expected [{B}, {gh}, {gw}] or [{B}, {P}])")
    if P > FAITHFULNESS_MAX_POSITIONS:
        raise ValueError(f"{what}: {P} grid positions, the ranking takes at most {FAITHFULNESS_MAX_POSITIONS}")


TOPK_MAX = 64   # include/vqa_hip.h vqa_softmax_topk: one wave keeps the k picks of a row, one per lane


def _check_k(what: str, k, A: int) -> int:
    if isinstance(k, bool) or not isinstance(k, int):
        raise ValueError(f"{what}: k must be an int, got {k!r}")
    if k < 1 or k > TOPK_MAX or k > A:
        raise ValueError(f"{what}: k={k} out of range (1 <= k <= min({TOPK_MAX}, number of answers = {A}))")
    return k


def topk_answers(logits, k: int = 1) -> TopAnswers:
    """The k best answers of every row of logits [B, A] -- what forward(), forward_shared() or answer() return -- with their
    softmax probabilities, ranked on the device in one kernel launch (csrc/topk.hip).

    Order: larger logit first; equal logits by smaller column; -0.0 equals +0.0; NaN ranks above +inf (torch.topk's
    order).  indices[:, 0] is therefore exactly the arg-max the library's VQA score is taken at (train.soft_ce_loss_and_score,
    torch.max's first maximum), which torch.topk does not promise on ties.  Columns are 0-based positions in the row: the
    loss head's a_idx is 1-based, so a_idx - 1 names the same answer.  probs = softmax(logits)[indices] in fp32; a row that
    contains NaN gets NaN probabilities.

    The result is detached (no autograd; a pending backward of `logits` stays usable).  ValueError for k < 1, k > A, k > 64
    or a tensor that is not 2-D, RuntimeError for a CPU tensor (there is no CPU fallback); a float dtype other than fp32 is
    widened with .float()."""
    logits = torch.as_tensor(logits)
    if logits.dim() != 2:
        raise ValueError(f"topk_answers: logits [B, A] expected, got {tuple(logits.shape)}")
    k = _check_k("topk_answers", k, logits.shape[1])
    if not logits.is_cuda:
        raise RuntimeError("dl_vqa_amd.topk_answers needs a CUDA (HIP) tensor; there is no CPU fallback")
    x = logits.detach()
    if x.dtype != torch.float32:
        x = x.float()
    if (x.shape[1] > 1 and x.stride(1) != 1) or (x.shape[0] > 1 and x.stride(0) < x.shape[1]):
        x = x.contiguous()                  # the kernel reads rows of unit stride, ld = stride(0) >= A apart
    return _ranked(x, k)


def _ranked(out, k: int):
    """TopAnswers of the fp32 CUDA logits `out`, ranked on their device; an (logits, attention) pair keeps its attention."""
    if isinstance(out, tuple):
        return _ranked(out[0], k), out[1]
    with torch.cuda.device(out.device):
        idx, prob = ops.softmax_topk(out, k)
    return TopAnswers(idx.long(), prob)


def _check_cache_dtype(what: str, dtype):
    """ValueError unless dtype is a storage format of ImageFeatures."""
    if dtype not in (torch.float32, torch.float16):
        raise ValueError(f"{what}: dtype must be torch.float32 or torch.float16 (the storage formats of image features), "
                         f"got {dtype!r}")


class ImageFeatures:
    """What VqaNet.encode_images returns and VqaNet.answer reads: the L2-normalised image features `vn` [N, P, C], their
    attention projection `vprime` = v_conv(vn) [N*P, mid], the grid (gh, gw) with P = gh * gw, and N.  A plain holder of
    CUDA tensors; it can be kept across many answer() calls, as long as the weights it was computed from stay the same.
    `vprime` is None for features encoded with with_vprime=False: a bank for VqaNet.forward_features, which reads `vn`
    alone (v' is 4x the size of vn in the reference's configuration and is recomputed there from the trained v_conv).

    Storage format (`dtype`): torch.float32, or torch.float16 = the fp32 features with each tensor rounded once to nearest
    even (encode_images(dtype=torch.float16), or .to(torch.float16)): half the bytes held and half the bytes every reader
    moves.  Every consumer widens on load and computes in fp32, so it gives, bit for bit, what it gives on the fp32 holder
    .to(torch.float32) of the same values; against the unrounded fp32 features the answers differ by that one rounding."""
    __slots__ = ("vn", "vprime", "grid", "N", "_model", "_flat_ptr")

    def __init__(self, vn, vprime, grid, model):
        self.vn, self.vprime, self.grid, self.N = vn, vprime, tuple(grid), vn.shape[0]
        self._model = weakref.ref(model)
        self._flat_ptr = model._flat_param.data_ptr()     # a re-flattened model (moved, new storage) no longer matches

    @property
    def dtype(self):
        """The storage format of vn (and of vprime, where there is one): torch.float32 or torch.float16."""
        return self.vn.dtype

    def to(self, dtype):
        """These features in the other storage format, as a new holder of the same model and grid (self for the same dtype).
        float32 -> float16 rounds both tensors once, with the library's converter (ops.to_half: to nearest even, as
        .half()); float16 -> float32 widens (ops.half_to_float), which is exact.  ValueError for any other dtype."""
        _check_cache_dtype("ImageFeatures.to", dtype)
        if dtype == self.dtype:
            return self
        with torch.cuda.device(self.vn.device):
            convert = ops.to_half if dtype == torch.float16 else ops.half_to_float
            out = ImageFeatures.__new__(ImageFeatures)
            out.vn = convert(self.vn.contiguous()) if self.vn.numel() else self.vn.to(dtype)
            out.vprime = None if self.vprime is None else (
                convert(self.vprime.contiguous()) if self.vprime.numel() else self.vprime.to(dtype))
        out.grid, out.N, out._model, out._flat_ptr = self.grid, self.N, self._model, self._flat_ptr
        return out

    @classmethod
    def cat(cls, parts):
        """Concatenate features of the same model and grid along N (a data set encoded in chunks): rows keep the order of
        `parts`.  vprime is concatenated when every part has one, otherwise the result has none.  TypeError for anything
        that is not an ImageFeatures, ValueError for an empty list, differing grids / feature widths or mixed storage
        formats (the result keeps the parts' common dtype), RuntimeError for
        parts of different models (or of a model whose parameters moved between two encode_images calls)."""
        parts = list(parts)
        if not parts:
            raise ValueError("ImageFeatures.cat: nothing to concatenate")
        for f in parts:
            if not isinstance(f, cls):
                raise TypeError("ImageFeatures.cat: every part must come from VqaNet.encode_images")
        first = parts[0]
        model = first._model()
        if model is None:
            raise RuntimeError("ImageFeatures.cat: the model that encoded these features no longer exists")
        for f in parts[1:]:
            if f._model() is not model or f._flat_ptr != first._flat_ptr:
                raise RuntimeError("ImageFeatures.cat: the parts were encoded by different models (or the model's parameters "
                                   "moved to new storage between the encode_images calls)")
            if f.grid != first.grid or f.vn.shape[1:] != first.vn.shape[1:] or f.vn.device != first.vn.device:
                raise ValueError(f"ImageFeatures.cat: grids / feature shapes differ ({first.grid} {tuple(first.vn.shape[1:])} "
                                 f"and {f.grid} {tuple(f.vn.shape[1:])})")
            if f.dtype != first.dtype:
                raise ValueError(f"ImageFeatures.cat: the parts have different storage formats ({first.dtype} and {f.dtype}); "
                                 "convert them with .to(dtype) first")
        vn = torch.cat([f.vn for f in parts], dim=0)
        vprime = torch.cat([f.vprime for f in parts], dim=0) if all(f.vprime is not None for f in parts) else None
        out = cls(vn, vprime, first.grid, model)
        out._flat_ptr = first._flat_ptr
        return out


class QuestionFeatures:
    """What VqaNet.encode_questions returns and VqaNet.answer_pairs reads: the question features `qf` [M, Q] (the LSTM's final
    cell states, what the classifier input holds behind the weighted image features; possibly a strided view), their attention
    projection `qprime` = q_lin(qf) [M, mid], and M.  A plain holder of CUDA tensors, owned like ImageFeatures: it belongs to
    the model that encoded it and to that model's current weights."""
    __slots__ = ("qf", "qprime", "M", "_model", "_flat_ptr")

    def __init__(self, qf, qprime, model):
        self.qf, self.qprime, self.M = qf, qprime, qf.shape[0]
        self._model = weakref.ref(model)
        self._flat_ptr = model._flat_param.data_ptr()


def unique_questions(q, q_len):
    """Deduplicate a batch of questions on the host: q [B, T] token ids, q_len [B] -> (q_unique [M, T], q_len_unique [M],
    question_index int64 [B]) with q_unique[question_index[b]] the question of row b.  Two questions are equal when their
    lengths and their first q_len tokens are equal (the recurrence never reads what lies behind q_len; the returned rows
    hold 0 there).  Distinct questions come in order of first occurrence.  CPU tensors come back, whatever device q was on;
    lengths below 1 or above T raise as validate_question_lengths does."""
    q = torch.as_tensor(q).detach().cpu()
    q_len = torch.as_tensor(q_len).detach().cpu()
    _check_question_ranks("unique_questions", q, q_len)
    B, T = q.shape
    validate_question_lengths(q_len, T)
    if B == 0:
        return q.clone(), q_len.clone(), torch.empty(0, dtype=torch.int64)
    masked = q * (torch.arange(T)[None, :] < q_len.to(torch.int64)[:, None]).to(q.dtype)
    keys = torch.cat([q_len.to(torch.int64)[:, None], masked.to(torch.int64)], dim=1)
    _, inverse = torch.unique(keys, dim=0, return_inverse=True)          # sorted groups; renumbered below
    M = int(inverse.max()) + 1
    first = torch.full((M,), B, dtype=torch.int64).scatter_reduce(0, inverse, torch.arange(B), reduce="amin")
    by_first = torch.argsort(first)                                      # group ids in order of first occurrence
    rank = torch.empty(M, dtype=torch.int64)
    rank[by_first] = torch.arange(M)
    rows = first[by_first]
    return masked[rows], q_len[rows], rank[inverse]


def _check_question_ranks(what: str, q, q_len, rows: str = "B", v=None):
    """ValueError unless q is [rows, T] and q_len [rows] (and the image batch v, where there is one, 4-D)."""
    if (v is not None and v.dim() != 4) or q.dim() != 2 or q_len.dim() != 1 or q_len.shape[0] != q.shape[0]:
        got = f"{tuple(q.shape)} and {tuple(q_len.shape)}"
        lead, got = ("v [N,3,S,S], ", f"{tuple(v.shape)}, " + got) if v is not None else ("", got)
        raise ValueError(f"{what}: {lead}q [{rows},T] and q_len [{rows}] expected, got {got}")


def _check_index_count(what: str, n_index: int, n: int, of: str = "questions"):
    """ValueError unless an index of n_index entries goes with n questions (or n entries of the other index)."""
    if n_index != n:
        raise ValueError(f"{what}: {n_index} image_index entries for {n} {of}")


def _need_cuda(what: str, on_device: bool):
    if not on_device:
        raise RuntimeError(f"dl_vqa_amd.VqaNet.{what} needs CUDA (HIP) tensors; there is no CPU fallback")


def _node_forward(ctx, model, run):
    """forward of an autograd node of this module: run(P) is the engine schedule, (logits, saved activations); the rest
    is what _node_backward and the model read afterwards."""
    logits, saved = run(model._param_dict())
    ctx.model = model
    ctx.saved = saved
    model._last_ctx = saved
    model._pending.add(ctx)          # weak: a graph that is dropped without backward leaves the set
    return logits


def _node_backward(ctx, dlogits, lead: int, engine_backward, frozen=()):
    """backward of an autograd node of this module (_VqaFunction, _VqaSharedFunction, _VqaFeaturesFunction): the
    gradient-buffer rules of _VqaFunction's docstring, once.  `lead`: how many inputs precede the parameters (input 1 is
    the image v); engine_backward(P, saved, dlogits, Gr, on_ready) is the engine schedule that matches the node's forward.
    `frozen`: names of parameters the schedule computes no gradient for -- they get None (autograd leaves their p.grad
    alone) and their slots of the gradient buffer are not written."""
    model = ctx.model
    if ctx.saved is None:
        raise RuntimeError("dl_vqa_amd.VqaNet: backward through the same forward twice (the saved "
                           "activations are released after the first backward; retain_graph is not supported)")
    names = model._names
    none_lead = (None,) * (lead - 2)
    if not any(ctx.needs_input_grad[lead:]):
        # every parameter frozen, only the image gradient is wanted: the parameter gradients go to a scratch buffer
        # (the model's flat gradient buffer, p.grad and the data-parallel buckets are left alone)
        _flat, Gr = model._grad_buffer(fresh=True)
        dv = engine_backward(model._param_dict(), ctx.saved, dlogits, Gr, None)
        ctx.saved = None
        model._pending.discard(ctx)
        return (None, dv) + none_lead + (None,) * len(names)
    others = [c for c in model._pending if c is not ctx]
    direct = not others and all(p.grad is None for p in model._params)
    if not direct and others and not model._warned_stale:
        model._warned_stale = True
        warnings.warn("dl_vqa_amd.VqaNet: backward runs while another grad-enabled forward of this module is still "
                      "waiting for its backward (an output kept for metrics / logging?): gradients go to a fresh "
                      "buffer instead of the model's flat gradient buffer (one extra buffer and, for FusedAdam, one "
                      "copy per step).  Use .detach() or torch.no_grad() for forwards that are never differentiated.")
    flat, Gr = model._grad_buffer(fresh=not direct)
    sync = model._grad_sync
    # data parallel: the SAME four bucket all-reduces, in the same order, from inside backward on either path
    # (a rank on the fresh-buffer path used to issue one whole-buffer collective against the other
    # ranks' four)
    on_ready = (lambda group: sync.bucket_ready(model, group, flat)) if sync is not None else None
    model._last_backward_direct = direct
    dv = engine_backward(model._param_dict(), ctx.saved, dlogits, Gr, on_ready)
    if sync is not None:
        sync.finish(model)
    ctx.saved = None
    model._pending.discard(ctx)
    return (None, dv) + none_lead + tuple(None if n in frozen else Gr[n] for n in names)


class _VqaFunction(torch.autograd.Function):
    """Autograd node of one VqaNet.forward call.

    Gradient storage: the model owns ONE flat gradient buffer (`_flat_grad`) that the fused optimiser
    and the data-parallel buckets work on.  backward writes into it directly -- and starts each
    bucket's all-reduce from inside backward -- only when that is safe: no parameter holds a gradient
    yet and no other forward of this module is still waiting for its backward (two forwards inside
    one graph would otherwise overwrite each other's gradients in place and autograd would then add
    two aliases of the same memory).  In every other case (gradient accumulation,
    ``zero_grad(set_to_none=False)``, several forwards per backward) the gradients go to a fresh
    buffer that autograd accumulates as usual; under data parallelism that buffer is all-reduced
    (through the same four bucket collectives, issued from inside backward in the same order) before it is handed
    to autograd, so replicas never step on unreduced gradients and the collective sequence is rank-invariant.
    """

    @staticmethod
    def forward(ctx, model, v, q, q_len, seed, *params):
        # v.requires_grad: the forward keeps what the first block's backward-data needs
        extra = {"need_dx": True} if ctx.needs_input_grad[1] else {}
        return _node_forward(ctx, model, lambda P: model._engine.forward(
            P, v, q, q_len, model.training, seed, keep=True, bad_tokens=model._token_counter(q), **extra))

    @staticmethod
    def backward(ctx, dlogits):
        return _node_backward(ctx, dlogits, 5, ctx.model._engine.backward)


class _VqaSharedFunction(torch.autograd.Function):
    """Autograd node of one VqaNet.forward_shared call: _VqaFunction with the image batch holding every image once.  index
    is the device int32 triple (order [B], offsets [N+1], image index [B]) of _upload_index; gradient storage follows
    _VqaFunction's rules through the same helper."""

    @staticmethod
    def forward(ctx, model, v, q, q_len, seed, index, *params):
        return _node_forward(ctx, model, lambda P: model._engine.forward_shared(
            P, v, q, q_len, *index, model.training, seed, keep=True, bad_tokens=model._token_counter(q),
            need_dx=bool(ctx.needs_input_grad[1])))

    @staticmethod
    def backward(ctx, dlogits):
        return _node_backward(ctx, dlogits, 6, ctx.model._engine.backward_grouped)


def _slot_of(index):
    """The slot view of forward_features' uploaded index (rows, order, offsets, img[, slot]): there with image dropout."""
    return index[4] if len(index) > 4 else None


class _VqaFeaturesFunction(torch.autograd.Function):
    """Autograd node of one VqaNet.forward_features call: the image encoder is not part of the graph.  vn is the bank's
    feature tensor (no gradient), index the device int32 views (rows [n_u], order [B], offsets [n_u+1], image index [B] and,
    with image dropout, slot [B]) of _upload_index.  Every parameter is an input, so that gradient storage follows
    _VqaFunction's rules through the same helper; the image.* parameters get None."""

    @staticmethod
    def forward(ctx, model, vn, q, q_len, seed, index, *params):
        return _node_forward(ctx, model, lambda P: model._engine.forward_features(
            P, vn, q, q_len, *index[:4], model.training, seed, keep=True, bad_tokens=model._token_counter(q), slot=_slot_of(index)))

    @staticmethod
    def backward(ctx, dlogits):
        model = ctx.model
        return _node_backward(ctx, dlogits, 6, model._engine.backward_grouped, model._image_names)


class VqaNet(nn.Module):
    """MI355X-native VqaNet (reference: models/model.py:7-67)."""

    def __init__(self, cfg, embedding_tokens, compute_dtype: str = "fp32"):
        """compute_dtype (not in the reference): "fp32" (default; the parity path, exact fp32 MFMA) or "bf16" (BASELINE
        configs[3]: conv blocks 1.. and the v_conv products on bf16 MFMA with fp32 accumulation; parameters, LSTM,
        reductions and Adam stay fp32)."""
        super().__init__()
        text_cfg, image_cfg = cfg["text"], cfg["image"]
        attention_cfg, classifier_cfg = cfg["attention"], cfg["classifier"]
        lstm_out_features = text_cfg["question_features"] * (2 if text_cfg["bidirectional"] else 1)
        glimpses = attention_cfg["glimpses"]
        image_features = image_cfg["num_channels"][-1]
        # same construction order as the reference => same RNG stream => identical initial weights
        self.text = questionNet(embedding_tokens=embedding_tokens,
                                embedding_features=text_cfg["embedding_features"],
                                lstm_features=text_cfg["question_features"], drop=text_cfg["dropout"],
                                num_lstm_layers=text_cfg["num_lstm_layers"],
                                bidirectional=text_cfg["bidirectional"])
        self.image = ImageNet2(image_cfg)
        self.attention = Attention(v_features=image_features, q_features=lstm_out_features,
                                   mid_features=attention_cfg["hidden_dim"], glimpses=glimpses,
                                   do_option=attention_cfg["do_option"], drop=attention_cfg["dropout"])
        self.classifier = Classifier(in_features=glimpses * image_features + lstm_out_features,
                                     mid_features=classifier_cfg["hidden_dim"], out_features=cfg["max_answers"],
                                     drop=classifier_cfg["dropout"])
        self.compute_dtype = compute_dtype
        self._engine = Engine(cfg, embedding_tokens, compute_dtype)
        named = OrderedDict(self.named_parameters())
        self._names: List[str] = list(named.keys())                    # state_dict order (autograd inputs)
        self._params: List[nn.Parameter] = list(named.values())
        self._flat_names = _flat_order(self._names)
        self._image_names = frozenset(n for n in self._names if n.startswith("image."))   # frozen in forward_features
        self._flat_param: Optional[torch.Tensor] = None
        self._flat_grad: Optional[torch.Tensor] = None
        self._offsets: Dict[str, tuple] = {}
        self._grad_sync = None          # set by dl_vqa_amd.distributed.DataParallel
        self._last_ctx = None
        self._seed_rank = 0
        self._pending = weakref.WeakSet()   # autograd nodes of forwards whose backward has not run yet
        self._warned_stale = False
        self._last_backward_direct = None   # did the last backward write the model's own flat buffer (bench, tests)
        self._bad_tokens = None             # device counter of out-of-vocabulary token ids (+ pinned host copy, event)
        self._bad_host = None
        self._bad_event = None

    # ------------------------------------------------------------------ flat parameter storage
    def _flatten(self, device):
        named = dict(zip(self._names, self._params))
        off = 0
        self._offsets = {}
        for n in self._flat_names:
            numel = named[n].numel()
            self._offsets[n] = (off, numel)
            off += (numel + 63) // 64 * 64            # 256-byte aligned starts (GEMM operands need 16 B)
        flat = torch.zeros(off, dtype=torch.float32, device=device)
        for n in self._flat_names:
            o, numel = self._offsets[n]
            p = named[n]
            view = flat[o:o + numel].view(p.shape)
            view.copy_(p.data)
            p.data = view
        self._flat_param = flat
        self._flat_grad = torch.zeros_like(flat)

    def _ensure_flat(self):
        dev = self._params[0].device
        if dev.type != "cuda":
            raise RuntimeError("dl_vqa_amd.VqaNet runs only on an MI355X: move the model with .cuda() "
                               "(there is no CPU fallback)")
        ok = self._flat_param is not None and self._flat_param.device == dev
        if ok:
            base = self._flat_param.data_ptr()
            for n, p in zip(self._names, self._params):
                if p.dtype != torch.float32 or p.data_ptr() != base + 4 * self._offsets[n][0]:
                    ok = False
                    break
        if not ok:
            self._flatten(dev)

    def _param_dict(self) -> Dict[str, torch.Tensor]:
        return {n: p.data for n, p in zip(self._names, self._params)}

    def _grad_buffer(self, fresh: bool = False):
        """(flat buffer, {name: view}) -- the model's own flat gradient buffer, or a fresh one of the same layout."""
        flat = torch.zeros_like(self._flat_grad) if fresh else self._flat_grad
        out = {}
        for n, p in zip(self._names, self._params):
            o, numel = self._offsets[n]
            out[n] = flat[o:o + numel].view(p.shape)
        return flat, out

    def _grad_views(self, fresh: bool = False) -> Dict[str, torch.Tensor]:
        return self._grad_buffer(fresh)[1]

    def flat_buffers(self):
        """(flat parameters, flat gradients, {name: (offset, numel)}) — used by the fused optimiser and DP."""
        self._ensure_flat()
        return self._flat_param, self._flat_grad, dict(self._offsets)

    def group_range(self, group: str):
        """Contiguous [lo, hi) range of the flat buffers that holds a backward group's parameters."""
        offs = [self._offsets[n] for n in self._flat_names if n.split(".")[0] == group]
        lo = min(o for o, _ in offs)
        hi = max(o + (k + 63) // 64 * 64 for o, k in offs)
        return lo, hi

    # ------------------------------------------------------------------ forward
    def _next_seed(self) -> int:
        # one draw from torch's CPU generator per training forward: reproducible under torch.manual_seed
        s = int(torch.empty((), dtype=torch.int64).random_().item())
        return (s ^ (self._seed_rank * 0x5851F42D4C957F2D)) & ((1 << 63) - 1)

    # ------------------------------------------------------------------ token-id validation
    # nn.Embedding raises for ids outside [0, V) (models/model.py:155).  Ids that arrive on the host are checked
    # there; ids already on the device are counted by the embedding kernel and the count is read back without
    # blocking: the error surfaces at the next forward (or at check_token_ids(), which synchronises) -- the
    # same deferred reporting a device-side assert has.
    def _validate_tokens(self, q):
        V = self._engine.V
        if not q.is_cuda:
            if q.numel() and (int(q.min()) < 0 or int(q.max()) >= V):
                raise IndexError(f"question token id out of range [0, {V}) (nn.Embedding would raise: models/model.py:155)")
            return
        self._raise_if_bad(block=False)
        dev = q.device
        if self._bad_tokens is None or self._bad_tokens.device != dev:
            self._bad_tokens = torch.zeros(1, dtype=torch.int32, device=dev)
            self._bad_host = torch.zeros(1, dtype=torch.int32).pin_memory()
            self._bad_event = None

    def _token_counter(self, q):
        """What the engine gets as bad_tokens: the device counter for ids that are on the device, nothing for ids that
        _validate_tokens has checked on the host."""
        return self._bad_tokens if q.is_cuda else None

    def _after_forward_tokens(self, q):
        if q.is_cuda and self._bad_tokens is not None:
            self._bad_host.copy_(self._bad_tokens, non_blocking=True)
            self._bad_event = torch.cuda.Event()
            self._bad_event.record(torch.cuda.current_stream(q.device))

    def _raise_if_bad(self, block: bool):
        ev = self._bad_event
        if ev is None:
            return
        if block:
            ev.synchronize()
        elif not ev.query():
            return
        self._bad_event = None
        n = int(self._bad_host[0])
        if n:
            self._bad_tokens.zero_()
            raise IndexError(f"{n} question token id(s) out of range [0, {self._engine.V}) in an earlier forward "
                             "(nn.Embedding would raise: models/model.py:155); they were embedded as zeros")

    def check_token_ids(self):
        """Synchronise and raise IndexError if a forward so far saw a token id outside the vocabulary."""
        self._raise_if_bad(block=True)

    def forward(self, v, q, q_len):
        self._ensure_flat()
        _need_cuda("forward", v.is_cuda)
        self._validate_tokens(q)
        validate_question_lengths(q_len, q.shape[1])
        # v may be the dataset's fp16 storage format (preprocessing/preprocess_images.py:39-53): the first-block kernels read
        # it as it is (engine.py); no widened copy is made
        if v.dtype not in (torch.float32, torch.float16):
            v = v.float()
        seed = self._next_seed() if self.training else 0
        # the autograd node also when only the image wants a gradient (saliency / attribution on a frozen model)
        need_grad = torch.is_grad_enabled() and (v.requires_grad or any(p.requires_grad for p in self._params))
        if need_grad:
            logits = _VqaFunction.apply(self, v, q, q_len, seed, *self._params)
        else:
            logits, _ = self._engine.forward(self._param_dict(), v, q, q_len, self.training, seed, keep=False,
                                             bad_tokens=self._token_counter(q))
        self._after_forward_tokens(q)
        return logits

    # ------------------------------------------------------------------ argument checks of the grouped paths
    def _refuse_bf16(self, what: str):
        if self.compute_dtype == "bf16":
            raise NotImplementedError(f"VqaNet.{what}: compute_dtype='bf16' is not supported (fp32 and fp32x3 are); the bf16 "
                                      "path rounds x = relu(v' (+|*) q') to bf16, a tensor this path never forms")

    def _check_grouped_training(self, what: str, how: str):
        self._refuse_bf16(what)
        if self._grad_sync is not None:
            raise NotImplementedError(f"VqaNet.{what}: data-parallel training {how} is not supported (the model is wrapped "
                                      "by dl_vqa_amd.distributed.DataParallel)")

    def _check_owned(self, what: str, held, kind: str, call: str):
        """RuntimeError unless the feature cache `held` (kind "image" / "question", made by `call`) belongs to this model and
        to its current parameter storage (after _ensure_flat)."""
        if held._model() is not self or held._flat_ptr != self._flat_param.data_ptr():
            raise RuntimeError(f"VqaNet.{what}: these {kind} features belong elsewhere -- they were encoded by another model "
                               "instance, or this model's parameters have moved to new storage since (.to(), a re-flatten); "
                               f"call {call} again on this model")

    def _no_answers(self, feats, return_attention: bool):
        """What answer / answer_pairs return for an empty batch."""
        eng, dev = self._engine, feats.vn.device
        logits = torch.empty(0, eng.A, dtype=torch.float32, device=dev)
        return (logits, torch.empty(0, eng.G, *feats.grid, dtype=torch.float32, device=dev)) if return_attention else logits

    # ------------------------------------------------------------------ training through shared image features
    def forward_shared(self, v, q, q_len, image_index):
        """forward() for a batch in which several questions ask about the same image: v [N,3,S,S] (fp32 or the dataset's
        fp16, CUDA) holds every image ONCE and question b (q[b], q_len[b]) looks at image image_index[b].  Returns logits
        [B, A]; B and N are independent.  The conv blocks and v_conv run once per image, forward and backward.

        image_index follows answer()'s rules: a host list or an integer tensor (a CUDA tensor is copied to the host, which
        synchronises once); repeats, any order and images nobody asks about are allowed; IndexError outside [0, N).

        Works in train and eval mode and is differentiable like forward(): the parameter gradients follow the same
        buffer rules (FusedAdam works unchanged), and with v.requires_grad the image gradient [N,3,S,S] comes back with
        the questions of an image summed.  Outside a grad context it returns the same logits and keeps nothing.

        Dropout in train mode departs from forward(v[image_index], ...) where sharing forces it: the image-side sites
        (image.drop, models/model.py:84, and attention.drop on v, model.py:185) draw one mask per IMAGE -- every question of
        an image sees the same dropped features -- while every question-side site (text, attention.drop on q and on x,
        both classifier sites) draws per question exactly as forward() does.  One seed is drawn per training forward.

        compute_dtype "bf16" and a model wrapped by dl_vqa_amd.distributed.DataParallel raise NotImplementedError."""
        self._check_grouped_training("forward_shared", "through shared image features")
        v, q, q_len = torch.as_tensor(v), torch.as_tensor(q), torch.as_tensor(q_len)
        _need_cuda("forward_shared", v.is_cuda)
        _check_question_ranks("VqaNet.forward_shared", q, q_len, v=v)
        B, N = q.shape[0], v.shape[0]
        img = _host_image_index(image_index, N)                      # the one copy to the host, reused below
        order, offsets = _group(img, N)
        _check_index_count("VqaNet.forward_shared", order.numel(), B)
        if N == 0 or B == 0:
            raise ValueError(f"VqaNet.forward_shared: an empty batch ({N} images, {B} questions)")
        self._ensure_flat()
        self._validate_tokens(q)
        validate_question_lengths(q_len, q.shape[1])
        if v.dtype not in (torch.float32, torch.float16):
            v = v.float()
        index = _upload_index(v.device, order, offsets, img)
        seed = self._next_seed() if self.training else 0
        need_grad = torch.is_grad_enabled() and (v.requires_grad or any(p.requires_grad for p in self._params))
        if need_grad:
            logits = _VqaSharedFunction.apply(self, v, q, q_len, seed, index, *self._params)
        else:
            logits, _ = self._engine.forward_shared(self._param_dict(), v, q, q_len, *index, self.training, seed, keep=False,
                                                    bad_tokens=self._token_counter(q))
        self._after_forward_tokens(q)
        return logits

    # ------------------------------------------------------------------ training on cached image features
    def forward_features(self, feats, q, q_len, image_index, image_dropout=False):
        """forward_shared() with the image encoder frozen and run beforehand: feats is an ImageFeatures of this model
        (encode_images, possibly with_vprime=False, possibly an ImageFeatures.cat of chunks) with N rows, and question b
        (q[b], q_len[b]) looks at row image_index[b].  Returns logits [B, A].  No convolution runs here, forward or
        backward, and only the rows that are asked about are touched: the cost does not depend on N.

        image_index follows answer()'s rules: a host list or an integer tensor (a CUDA tensor is copied to the host, which
        synchronises once); repeats, any order and rows nobody asks about are allowed; IndexError outside [0, N).

        Works in train and eval mode and is differentiable with respect to every parameter of text, attention (v_conv,
        q_lin, x_conv) and classifier; their gradients follow forward()'s buffer rules (FusedAdam works unchanged).  The
        parameters under image. are not part of the graph: their p.grad stays None, their slots of the flat gradient
        buffer are not written, and FusedAdam skips them.  Outside a grad context it returns the same logits and keeps
        nothing.  Only feats.vn is read: v' = v_conv(vn) is recomputed every step from the current v_conv.weight, so
        in-place optimiser steps never make feats stale for THIS call (they do for answer(), see encode_images).  feats
        must belong to this model instance and its current parameter storage, as for answer().  A float16 bank
        (feats.dtype == torch.float16) is read as it is -- the gather and the weighted sum widen on load -- and gives the
        logits and gradients of the fp32 bank holding the same values, bit for bit.

        Dropout in train mode: with image_dropout=False (the default) image.drop (models/model.py:84) is NOT applied -- the
        features are the encoder's eval-mode output.  image_dropout=True applies it at the configured rate, from the bank
        alone: the reference drops first and L2-normalises second (model.py:55-56), normalisation is scale-invariant, so the
        asked rows are masked and renormalised, m*vn / |m*vn| = m*pooled / |m*pooled|, in the pass that gathers them -- what
        the train-mode encoder would give for that mask, up to how the 1e-12 guard of the norm scales (immaterial unless the
        kept part of a feature row has a norm near 1e-12; an all-zero kept part gives zeros either way).  The mask is drawn
        per feature ROW of the bank, logical tensor [feats.N, gh, gw, C] at the image site, as attention.drop's below:
        forward_shared's convention for the same images in the same order, so with image_dropout=True
        forward_features(encode_images(v), ...) and forward_shared(v, ...) are the same function of the seed for the non-image
        parameters, up to rounding.  In eval mode, or with image.dropout = 0, True runs exactly what False runs.
        image_dropout must be a bool (ValueError otherwise, before any device work).  The image.* gradients stay None.

        attention.drop on v (model.py:185) draws one mask per feature ROW of the bank: the logical tensor is
        [feats.N, gh, gw, C], element (n, p, c) at flat index (n*P + p)*C + c with n the row in feats, not the slot in the
        batch -- forward_shared's convention for the same images in the same order, so with image.dropout = 0 the two calls
        are the same function of the seed.  Every question-side site (text, attention.drop
        on q and on x, both classifier sites) draws per question exactly as forward_shared does.  One seed is drawn per
        training forward, none in eval mode, with or without image_dropout.

        NotImplementedError for compute_dtype "bf16" and for a model wrapped by dl_vqa_amd.distributed.DataParallel,
        TypeError for a feats that is not an ImageFeatures, RuntimeError for CPU tensors or foreign features, ValueError
        for wrong ranks, a wrong image_index count or an empty batch."""
        if not isinstance(image_dropout, bool):
            raise ValueError(f"VqaNet.forward_features: image_dropout must be a bool, got {image_dropout!r}")
        self._check_grouped_training("forward_features", "on cached image features")
        if not isinstance(feats, ImageFeatures):
            raise TypeError("VqaNet.forward_features: feats must come from VqaNet.encode_images (or ImageFeatures.cat)")
        q, q_len = torch.as_tensor(q), torch.as_tensor(q_len)
        _need_cuda("forward_features", feats.vn.is_cuda and self._params[0].is_cuda)
        _check_question_ranks("VqaNet.forward_features", q, q_len)
        self._ensure_flat()
        self._check_owned("forward_features", feats, "image", "encode_images")
        B, N = q.shape[0], feats.N
        img = _host_image_index(image_index, N)                      # the one copy to the host, reused below
        rows, slot, order, offsets = compact_image_index(img, N)
        _check_index_count("VqaNet.forward_features", order.numel(), B)
        if N == 0 or B == 0:
            raise ValueError(f"VqaNet.forward_features: an empty batch ({N} feature rows, {B} questions)")
        self._validate_tokens(q)
        validate_question_lengths(q_len, q.shape[1])
        # image dropout at a rate above 0: the weighted sum then reads the dropped rows at a question's slot in `rows`
        drop = image_dropout and self.training and self._engine.p_image > 0
        index = _upload_index(feats.vn.device, rows, order, offsets, img, *((slot,) if drop else ()))
        seed = self._next_seed() if self.training else 0
        need_grad = torch.is_grad_enabled() and any(p.requires_grad for n, p in zip(self._names, self._params)
                                                    if n not in self._image_names)
        if need_grad:
            logits = _VqaFeaturesFunction.apply(self, feats.vn, q, q_len, seed, index, *self._params)
        else:
            logits, _ = self._engine.forward_features(self._param_dict(), feats.vn, q, q_len, *index[:4], self.training, seed,
                                                      keep=False, bad_tokens=self._token_counter(q), slot=_slot_of(index))
        self._after_forward_tokens(q)
        return logits

    # ------------------------------------------------------------------ many questions per image (inference)
    def _check_inference(self, what: str):
        self._refuse_bf16(what)
        if self.training:
            raise RuntimeError(f"VqaNet.{what} is an inference call and the model is in training mode: the image, attention "
                               "and classifier dropout sites (models/model.py:84,185,186,194) draw a new mask per forward, so "
                               "image features cached across questions would be meaningless; call model.eval() first")

    @staticmethod
    def _need_image_features(what: str, feats):
        if not isinstance(feats, ImageFeatures):
            raise TypeError(f"VqaNet.{what}: feats must come from VqaNet.encode_images")

    @staticmethod
    def _need_vprime(what: str, feats):
        if feats.vprime is None:
            raise RuntimeError(f"VqaNet.{what}: these image features were encoded with with_vprime=False (a bank for "
                               "forward_features: vn only); encode them with with_vprime=True to answer from them")

    @torch.no_grad()
    def encode_images(self, v, with_vprime: bool = True, dtype: torch.dtype = torch.float32) -> ImageFeatures:
        """The image-only part of the forward, once per image: conv blocks, L2 normalisation and v' = v_conv(vn).
        v [N,3,S,S] fp32 or fp16, CUDA.  Eval mode, compute_dtype fp32 or fp32x3; no autograd graph.

        dtype: the storage format of the result, torch.float32 (default) or torch.float16; anything else is a ValueError,
        raised before any device work.  float16 holds exactly encode_images(v).vn.half() and .vprime.half(): everything is
        computed in fp32 as for the default -- v' from the fp32 vn, not from the rounded one -- and each tensor is rounded
        once, to nearest even.  Half the memory, for an answer cache and for a training bank alike; answer, predict,
        answer_pairs, predict_pairs and forward_features read it as it is (see ImageFeatures).  The fp32 temporaries are
        this call's, so encoding in chunks keeps them at chunk size.

        with_vprime=False skips the v_conv product and leaves feats.vprime None: a bank for forward_features, which reads
        vn alone (chunks are joined by ImageFeatures.cat).  answer / predict / answer_pairs raise RuntimeError on it.

        The result belongs to this model and to its current weights.  answer() refuses features of another model instance
        or of a model whose parameters have moved to new storage, but it cannot see weights that changed IN PLACE (FusedAdam
        steps the flat parameter buffer through raw pointers; load_state_dict copies into it): re-encode after an
        optimiser step or load_state_dict."""
        _check_cache_dtype("VqaNet.encode_images", dtype)
        self._check_inference("encode_images")
        self._ensure_flat()
        _need_cuda("encode_images", v.is_cuda)
        if v.dtype not in (torch.float32, torch.float16):
            v = v.float()
        vn, vprime, grid = self._engine.encode_images(self._param_dict(), v.detach(), with_vprime=bool(with_vprime), dtype=dtype)
        return ImageFeatures(vn, vprime, grid, self)

    @torch.no_grad()
    def answer(self, feats: ImageFeatures, q, q_len, image_index, return_attention: bool = False):
        """Logits [B, A] of B questions about the N encoded images: question b (q[b], q_len[b]) looks at image
        image_index[b].  B and N are independent; any order of image_index, repeats and images nobody asks about
        included; rows come back in the caller's question order.  return_attention: also att [B, G, gh, gw] =
        softmax over positions of the attention scores, the weights the image features are summed with
        (models/model.py:217), on the feature grid (no upsampling).

        image_index is host data (a list or a CPU integer tensor); a CUDA tensor is copied to the host first, which
        synchronises once.  Nothing is kept for a backward: _last_ctx, the gradient buffer and the dropout seed stream are
        left alone.  See encode_images for when `feats` has to be recomputed."""
        self._check_inference("answer")
        q, q_len, index = self._answer_args("answer", feats, q, q_len, image_index)
        B = q.shape[0]
        if B == 0:
            return self._no_answers(feats, return_attention)
        eng = self._engine
        logits, probs, _score = eng.answer(self._param_dict(), feats, q, q_len, *_upload_index(feats.vn.device, *index),
                                           bad_tokens=self._token_counter(q))
        self._after_forward_tokens(q)
        if return_attention:
            return logits, probs.view(B, eng.G, *feats.grid)
        return logits

    def _answer_args(self, what: str, feats, q, q_len, image_index):
        """What answer() and explain() check after _check_inference, in answer()'s order.  Returns (q, q_len as tensors, the
        host index tensors (order, offsets, img) of the questions grouped by image)."""
        self._ensure_flat()
        self._need_image_features(what, feats)
        self._check_owned(what, feats, "image", "encode_images")
        self._need_vprime(what, feats)
        q = torch.as_tensor(q)
        q_len = torch.as_tensor(q_len)
        _check_question_ranks(f"VqaNet.{what}", q, q_len)
        self._validate_tokens(q)
        validate_question_lengths(q_len, q.shape[1])
        B, N = q.shape[0], feats.N
        img = _host_image_index(image_index, N)                      # the one copy to the host, reused below
        order, offsets = _group(img, N)
        _check_index_count(f"VqaNet.{what}", order.numel(), B)
        return q, q_len, (order, offsets, img)

    @torch.no_grad()
    def predict(self, feats: ImageFeatures, q, q_len, image_index, k: int = 1, return_attention: bool = False):
        """answer() and the ranking of its logits in one call: TopAnswers(indices int64 [B, k], probs fp32 [B, k]), the k best
        answers of every question and their softmax probabilities, best first, in topk_answers' order (larger logit first,
        equal logits by smaller column: indices[:, 0] is the arg-max the VQA score is taken at; 0-based, a_idx - 1).
        return_attention: (TopAnswers, att [B, G, gh, gw]) with answer()'s attention tensor.

        k is validated first (ValueError for k < 1, k > 64 or k > the number of answers); everything else is answer()'s:
        eval mode only, fp32 / fp32x3, the feature-ownership checks, its errors, and nothing kept for a backward.  The
        ranking kernel runs on answer()'s device and stream, behind the classifier; B == 0 gives empty [0, k] tensors."""
        k = _check_k("VqaNet.predict", k, self._engine.A)
        return _ranked(self.answer(feats, q, q_len, image_index, return_attention=return_attention), k)

    # ------------------------------------------------------------------ cached question features (inference)
    @torch.no_grad()
    def encode_questions(self, q, q_len) -> QuestionFeatures:
        """The question-only part of the forward, once per question: embedding, the LSTM and q' = q_lin(qf).  q [M,T] token
        ids, q_len [M] (host or CUDA).  Eval mode, compute_dtype fp32 or fp32x3; no autograd graph.  Token ids and lengths
        are validated as answer() validates them; M == 0 gives empty features.

        The result belongs to this model and to its current weights, exactly as encode_images' does: answer_pairs()
        refuses features of another model instance or of moved parameters, but cannot see weights that changed IN PLACE --
        re-encode after an optimiser step or load_state_dict.  dl_vqa_amd.unique_questions deduplicates a batch first."""
        self._check_inference("encode_questions")
        self._ensure_flat()
        q = torch.as_tensor(q)
        q_len = torch.as_tensor(q_len)
        _check_question_ranks("VqaNet.encode_questions", q, q_len, rows="M")
        self._validate_tokens(q)
        validate_question_lengths(q_len, q.shape[1])
        dev = self._flat_param.device
        eng = self._engine
        if q.shape[0] == 0:
            return QuestionFeatures(torch.empty(0, eng.Q, dtype=torch.float32, device=dev),
                                    torch.empty(0, eng.mid, dtype=torch.float32, device=dev), self)
        qf, qprime = eng.encode_questions(self._param_dict(), q.detach(), q_len.detach(), dev,
                                          bad_tokens=self._token_counter(q))
        self._after_forward_tokens(q)
        return QuestionFeatures(qf, qprime, self)

    @torch.no_grad()
    def answer_pairs(self, feats: ImageFeatures, qfeats: QuestionFeatures, image_index, question_index,
                     return_attention: bool = False):
        """Logits [B, A] of B (image, question) pairs from the two caches: pair b looks at image image_index[b] of `feats`
        (encode_images) with question question_index[b] of `qfeats` (encode_questions).  No recurrence and no convolution
        runs here.  Both indices follow answer()'s rules for image_index: host lists or integer tensors (a CUDA tensor is
        copied to the host, which synchronises once), any order, repeats, and unused images or questions allowed.
        return_attention: also att [B, G, gh, gw], as from answer().

        ValueError when the indices differ in length, IndexError outside [0, N) / [0, M), TypeError for anything that did
        not come from encode_images / encode_questions, RuntimeError when a cache belongs to another model instance, to
        moved parameters, or to another device than the other cache.  Nothing is kept for a backward: _last_ctx, the
        gradient buffer and the dropout seed stream are left alone."""
        self._check_inference("answer_pairs")
        index = self._pairs_args("answer_pairs", feats, qfeats, image_index, question_index)
        eng = self._engine
        B = index[-1].numel()
        if B == 0:
            return self._no_answers(feats, return_attention)
        logits, probs, _score = eng.answer_pairs(self._param_dict(), feats, qfeats, *_upload_index(feats.vn.device, *index))
        if return_attention:
            return logits, probs.view(B, eng.G, *feats.grid)
        return logits

    def _pairs_args(self, what: str, feats, qfeats, image_index, question_index):
        """What answer_pairs() and explain_pairs() check after _check_inference, in answer_pairs()'s order.  Returns the host
        index tensors (order, offsets, img, qidx) of the pairs grouped by image."""
        self._need_image_features(what, feats)
        if not isinstance(qfeats, QuestionFeatures):
            raise TypeError(f"VqaNet.{what}: qfeats must come from VqaNet.encode_questions")
        N, M = feats.N, qfeats.M
        n_img, n_q = torch.as_tensor(image_index).numel(), torch.as_tensor(question_index).numel()
        _check_index_count(f"VqaNet.{what}", n_img, n_q, "question_index entries")
        img = _host_image_index(image_index, N)                      # each index: one copy to the host, reused below
        order, offsets = _group(img, N)
        qidx = _host_image_index(question_index, M, "question_index", "questions")
        self._ensure_flat()
        self._check_owned(what, feats, "image", "encode_images")
        self._check_owned(what, qfeats, "question", "encode_questions")
        self._need_vprime(what, feats)
        dev = feats.vn.device
        if qfeats.qprime.device != dev:
            raise RuntimeError(f"VqaNet.{what}: the image features are on {dev} and the question features on "
                               f"{qfeats.qprime.device}; encode both on the model's device")
        return order, offsets, img, qidx

    @torch.no_grad()
    def predict_pairs(self, feats: ImageFeatures, qfeats: QuestionFeatures, image_index, question_index, k: int = 1,
                      return_attention: bool = False):
        """answer_pairs() and the ranking of its logits in one call, as predict() wraps answer(): TopAnswers(indices int64
        [B, k], probs fp32 [B, k]) in topk_answers' order; return_attention: (TopAnswers, att [B, G, gh, gw]).  k is
        validated first; everything else is answer_pairs()'s."""
        k = _check_k("VqaNet.predict_pairs", k, self._engine.A)
        return _ranked(self.answer_pairs(feats, qfeats, image_index, question_index, return_attention=return_attention), k)

    # ------------------------------------------------------------------ gradient x input maps from cached features
    def _answer_columns(self, what: str, answers, B: int):
        """The `answers` argument of explain / explain_pairs, judged on the host: None (each question's arg-max), a CUDA
        integer tensor of B columns as it is, or host data as int32 [B] after its range check."""
        if answers is None:
            return None
        cols = torch.as_tensor(answers).detach().reshape(-1)
        if cols.is_floating_point() or cols.is_complex() or cols.dtype == torch.bool:
            raise TypeError(f"VqaNet.{what}: answers must hold integer answer columns, got {cols.dtype}")
        if cols.numel() != B:
            raise ValueError(f"VqaNet.{what}: {cols.numel()} answers for {B} questions")
        if cols.is_cuda:
            return cols
        A = self._engine.A
        if B and (int(cols.min()) < 0 or int(cols.max()) >= A):
            bad = int(cols.min()) if int(cols.min()) < 0 else int(cols.max())
            raise IndexError(f"VqaNet.{what}: answers entry {bad} out of range [0, {A})")
        return cols.to(torch.int32)

    # The front door of the explain family.  Every call asks (_ask_questions / _ask_pairs: all the argument checks, on the
    # host), returns _no_result for an empty batch, uploads (_ask_upload: the index, host answers and the call's own host
    # tensors in ONE copy), runs its engine schedule (_ask_run) and wraps what comes back.  A public call binds its arguments
    # to one of the two doors and hands the door to its member, which is written once for both (_explain_member).
    def _ask_questions(self, what: str, feats, q, q_len, image_index, answers, own=None, host_first: bool = False):
        """What an explain call about (q, q_len, image_index) checks, in order: the inference check, the call's `own` check
        (explain_occlusion's window: own(the call's full name, B), whose value the ask keeps as .own), the type of feats, the
        `answers` columns, then _answer_args.  host_first (explain_words,
        explain_words_occlusion): what the host alone can judge -- a bank without v', the index count -- comes before
        `answers`, in _answer_args' words.  Returns the ask: B, q / q_len as tensors, the host index tensors, the columns."""
        self._check_inference(what)
        checked = None if own is None else own(f"VqaNet.{what}", len(q))
        self._need_image_features(what, feats)
        if host_first:
            self._need_vprime(what, feats)
            _check_index_count(f"VqaNet.{what}", torch.as_tensor(image_index).numel(), len(q))
        cols = self._answer_columns(what, answers, len(q))
        q, q_len, index = self._answer_args(what, feats, q, q_len, image_index)
        return SimpleNamespace(B=q.shape[0], q=q, q_len=q_len, qfeats=None, index=index, cols=cols, own=checked)

    def _ask_pairs(self, what: str, feats, qfeats, image_index, question_index, answers, own=None):
        """_ask_questions for (image, question) pairs from the two caches: the inference check, `own`, the `answers` columns,
        then _pairs_args.  The ask holds qfeats in place of q / q_len, and the host index has the question rows behind img."""
        self._check_inference(what)
        B = torch.as_tensor(image_index).numel()
        checked = None if own is None else own(f"VqaNet.{what}", B)
        cols = self._answer_columns(what, answers, B)
        index = self._pairs_args(what, feats, qfeats, image_index, question_index)
        return SimpleNamespace(B=index[-1].numel(), q=None, q_len=None, qfeats=qfeats, index=index, cols=cols, own=checked)

    def _ask_upload(self, feats, ask, extra=()):
        """The ask on the device of feats, as the engine reads it: on_device, the index tensors, and answers as int32, and
        bad_tokens.  `extra`: the call's own host index tensors, which travel in the same single copy; their device views are
        returned in the same order."""
        n = len(ask.index)
        index, ask.answers = _upload_with_columns(feats.vn.device, tuple(ask.index) + tuple(extra), ask.cols)
        ask.on_device = index[:n]
        ask.bad_tokens = self._token_counter(ask.q) if ask.q is not None else None
        return index[n:]

    def _ask_upload_asked(self, feats, ask, extra=(), grouped: bool = False):
        """_ask_upload for the calls that explain sets of grid positions: the distinct asked images and each question's place
        among them (compact_image_index) travel in the copy in front of `extra`.  Returns (rows, slot, *extra) on the device;
        grouped (explain_faithfulness_probs): by_slot travels behind slot, and ask.offsets is the host list of the grouping."""
        rows, slot, by_slot, offsets = compact_image_index(ask.index[2], feats.N)
        ask.offsets = offsets.tolist()
        return self._ask_upload(feats, ask, (rows, slot) + ((by_slot,) if grouped else ()) + tuple(extra))

    @staticmethod
    def _device_maps(feats, ask, maps):
        """The caller's maps as the engine reads them: fp32 [B, P], contiguous, on the device of feats."""
        return torch.as_tensor(maps).detach().to(device=feats.vn.device, dtype=torch.float32).reshape(ask.B, -1).contiguous()

    def _explain_member(self, door, feats, kind, own, member):
        """An explain call behind its door (_ask_questions or _ask_pairs, everything but `own` bound): the ask, judged with the
        member's host-only check `own`; `kind` with every field empty for B == 0; else member(ask) -- the member's upload, its
        engine schedule and its result."""
        ask = door(own=own)
        if ask.B == 0:
            return self._no_result(kind, feats, 0 if ask.q is None else ask.q.shape[1])
        return member(ask)

    def _ask_run(self, schedule, feats, ask, *args):
        """The engine schedule on an uploaded ask, and the token count read back where question tokens were embedded."""
        out = schedule(self._param_dict(), feats, ask, *args)
        if ask.q is not None:
            self._after_forward_tokens(ask.q)
        return out

    def _no_result(self, kind, feats, T: int = 0):
        """What an explain call returns for B == 0: the result type `kind` with every field empty."""
        P = feats.grid[0] * feats.grid[1]
        shape = dict(words=(0, T), maps=(0, *feats.grid), stderr=(0, *feats.grid), answers=(0,), logits=(0, self._engine.A),
                     deletion=(0, P + 1), insertion=(0, P + 1), order=(0, P), baseline_logits=(0,))
        shape.update({f: (0, P + 1) for f in ("deletion_top", "insertion_top", "deletion_top_prob", "insertion_top_prob")})
        dtype = lambda f: torch.int64 if f in ("answers", "order") else torch.int32 if f.endswith("_top") else torch.float32
        return kind(*(torch.empty(shape[f], dtype=dtype(f), device=feats.vn.device) for f in kind._fields))

    @staticmethod
    def _maps_result(kind, feats, out):
        """Attribution / Occlusion of the engine's (maps [B,P], answers int32 [B], logits)."""
        maps, cols, logits = out
        return kind(maps.view(-1, *feats.grid), cols.long(), logits)

    @torch.no_grad()
    def explain(self, feats: ImageFeatures, q, q_len, image_index, answers=None) -> Attribution:
        """answer() with a gradient x input map per question: Attribution(maps fp32 [B, gh, gw], answers int64 [B], logits
        fp32 [B, A]).  For question b about image n = image_index[b] and the answer column a_b = answers[b],

            maps[b, p] = R[b, p] = sum_c vn[n, p, c] * d logits[b, a_b] / d vn[n, p, c]

        on the feature grid: signed, not upsampled, not normalised.  R is the attribution AT THE NORMALISED FEATURE LAYER
        (feats.vn, the output of the conv blocks after the L2 normalisation) WITH THE QUESTION HELD FIXED: it follows vn
        along both of its paths to the logit -- the attention-weighted sum, and the attention scores through v_conv -- in
        eval mode.  The conv blocks, the L2 normalisation and the question path (embedding, LSTM, q_lin, the question half
        of the classifier input) are not part of it: nothing is attributed to pixels or to question tokens.  No convolution
        and no v_conv product runs, and the gradient tensor itself is never formed (include/vqa_hip.h has the formulas).

        answers=None explains each question's arg-max answer, chosen on the device in topk_answers' order (ties by the
        smaller column): answers == predict(feats, q, q_len, image_index, k=1).indices[:, 0].  Otherwise answers is a list or
        an integer tensor of B columns (0-based, as TopAnswers.indices).  Host data is checked: ValueError for a wrong count,
        IndexError outside [0, A), TypeError for a non-integer dtype.  A CUDA tensor is taken as it is, without a copy to the
        host: its count is checked, its values are not, and an entry outside [0, A) gives a map of zeros.

        logits are answer()'s for the same arguments, bit for bit.  Everything else is answer()'s too: eval mode only
        (RuntimeError in train mode), fp32 / fp32x3 (NotImplementedError for "bf16"), both judged before any device work;
        the feature-ownership checks and image_index rules; fp32 and float16 caches (a float16 cache gives, bit for bit,
        what feats.to(torch.float32) gives); B == 0 returns empty tensors.  Rows come back in the caller's order and do not
        depend on how the batch is ordered or split.  Nothing is kept for a backward: _last_ctx, the gradient buffer, p.grad
        and the dropout seed stream are left alone."""
        return self._explain(partial(self._ask_questions, "explain", feats, q, q_len, image_index, answers), feats)

    def _explain(self, door, feats) -> Attribution:
        def member(ask):
            self._ask_upload(feats, ask)
            return self._maps_result(Attribution, feats, self._ask_run(self._engine.explain, feats, ask))
        return self._explain_member(door, feats, Attribution, None, member)

    @torch.no_grad()
    def explain_pairs(self, feats: ImageFeatures, qfeats: QuestionFeatures, image_index, question_index,
                      answers=None) -> Attribution:
        """explain() for B (image, question) pairs from the two caches, as answer_pairs() is to answer(): pair b looks at
        image image_index[b] of `feats` with question question_index[b] of `qfeats`; no recurrence runs either.  maps, answers
        and the `answers` argument are explain()'s; logits are answer_pairs()'s for the same arguments, bit for bit; the index
        rules, ownership checks and errors are answer_pairs()'s, with the `answers` checks of explain() judged first."""
        return self._explain(partial(self._ask_pairs, "explain_pairs", feats, qfeats, image_index, question_index, answers), feats)

    # ------------------------------------------------------------------ integrated gradients from cached features
    @torch.no_grad()
    def explain_integrated(self, feats: ImageFeatures, q, q_len, image_index, answers=None, steps: int = 16, *,
                           _ig_bytes=None) -> IntegratedGradients:
        """answer() with an integrated-gradients map per question: IntegratedGradients(maps fp32 [B, gh, gw], answers int64
        [B], logits fp32 [B, A], baseline_logits fp32 [B]).  For question b about image n = image_index[b] and the answer column
        a_b = answers[b], with explain()'s map R evaluated on a scaled cache,

            G_s[b, p]  = sum_c vn[n, p, c] * d logits[b, a_b] / d x[p, c]     at x = alpha_s * vn[n]
            maps[b, p] = (1 / steps) * sum_s G_s[b, p]                        alpha_s = float32((2s + 1) / (2 * steps))

        the midpoint-rule Riemann sum of the gradient along the straight path from an image cache of ZEROS to the real one, eval
        mode, the question held fixed (v_conv has no bias, so scaling vn scales v').  explain()'s gradient x input map is the
        one-point rule at alpha = 1 and misses logits[b, a_b] - baseline_logits[b] by tens of per cent of it;
        these maps sum to that difference up to the quadrature error, which completeness_gap() returns and which falls as steps
        grows (first order only: the ReLUs put kinks on the path).  The midpoint rule never evaluates alpha = 0, where '*' and
        '|' have every pre-activation exactly zero.  baseline_logits[b] is the eval-mode classifier on [0, question features].

        steps: an int in 1..64 (default 16); anything else, a bool included, is a ValueError raised before any device work.

        How it runs.  Composing it from explain() reads v' from memory 2 * steps times and runs the question encoder steps
        times.  Here the question encoder, q_lin and answer()'s tail run once; two kernels walk v' once each whatever steps is
        (include/vqa_hip.h vqa_att_path_score_grouped, vqa_att_path_attr_grouped: a tile of v' staged once serves every question
        of the image and every step), and the softmax, the weighted sum and the classifier's first layer run on the B * steps
        step-rows between them, in chunks of questions whose buffers stay within a 256 MiB workspace.  No parameter gradient is
        formed and nothing is kept.

        answers, logits, the `answers` argument, the argument rules and the refusals are explain()'s, judged before any device
        work: eval mode only (RuntimeError in train mode), fp32 / fp32x3 (NotImplementedError for "bf16"), features that hold
        v', the feature-ownership checks and image_index rules; all three do_option values; fp32 and float16 caches (a float16
        cache gives, bit for bit, what feats.to(torch.float32) gives); a CUDA `answers` entry outside [0, A) gives a map of
        zeros and a zero baseline; B == 0 returns empty tensors.  Rows come back in the caller's order and do not depend on how
        the batch is ordered, split or chunked, bit for bit.

        Not offered: other baselines (mean or blurred features), other quadratures, integrated gradients for the words or the
        pixels, SmoothGrad, bf16 mode, train mode, data parallelism.

        _ig_bytes (tests and tools): the workspace cap in bytes, to force several chunks at small sizes."""
        door = partial(self._ask_questions, "explain_integrated", feats, q, q_len, image_index, answers)
        return self._explain_integrated(door, feats, steps, _ig_bytes)

    def _explain_integrated(self, door, feats, steps, ig_bytes) -> IntegratedGradients:
        def member(ask):
            # chunks cut between questions, in the caller's order; a single chunk walks the ask's own grouping
            rows = self._engine.integrated_rows(feats.vn.shape[1], ask.own, ig_bytes)
            cuts = [(b0, min(b0 + rows, ask.B)) for b0 in range(0, ask.B, rows)]
            img = ask.index[2]
            groups = [t for b0, b1 in cuts for t in _group(img[b0:b1], feats.N)] if len(cuts) > 1 else []
            on_device = self._ask_upload(feats, ask, groups) or ask.on_device[:2]
            chunks = [(b0, b1, on_device[2 * i], on_device[2 * i + 1]) for i, (b0, b1) in enumerate(cuts)]
            alphas = integrated_alphas(ask.own).to(feats.vn.device)
            maps, cols, logits, base = self._ask_run(self._engine.explain_integrated, feats, ask, alphas, chunks)
            return IntegratedGradients(maps.view(-1, *feats.grid), cols.long(), logits, base)
        return self._explain_member(door, feats, IntegratedGradients, lambda what, B: _check_steps(what, steps), member)

    @torch.no_grad()
    def explain_integrated_pairs(self, feats: ImageFeatures, qfeats: QuestionFeatures, image_index, question_index,
                                 answers=None, steps: int = 16, *, _ig_bytes=None) -> IntegratedGradients:
        """explain_integrated() for B (image, question) pairs from the two caches, as answer_pairs() is to answer(): pair b
        looks at image image_index[b] of `feats` with question question_index[b] of `qfeats`; no recurrence runs either.  maps,
        answers, baseline_logits, steps and the `answers` argument are explain_integrated()'s; logits are answer_pairs()'s for
        the same arguments, bit for bit; the index rules, ownership checks and errors are answer_pairs()'s, with the steps and
        `answers` checks judged first."""
        door = partial(self._ask_pairs, "explain_integrated_pairs", feats, qfeats, image_index, question_index, answers)
        return self._explain_integrated(door, feats, steps, _ig_bytes)

    # ------------------------------------------------------------------ occlusion maps from cached features
    @torch.no_grad()
    def explain_occlusion(self, feats: ImageFeatures, q, q_len, image_index, answers=None, window: int = 1, *,
                          _u_bytes=None) -> Occlusion:
        """answer() with an occlusion map per question: Occlusion(maps fp32 [B, gh, gw], answers int64 [B], logits fp32
        [B, A]).  For question b about image n = image_index[b] and the answer column a_b = answers[b],

            maps[b, p] = logits[b, a_b] - logit_occluded[b, a_b; S(p)]

        where S(p) is the window x window square of grid positions centred on p, clipped at the grid border, and "occluded"
        means that the L2-normalised features vn[n, s, :] of every s in S(p) are zero (hence v'[n, s, :] too: v_conv has no
        bias) -- exactly what answer() computes on a cache whose rows s are zeroed in vn and in v'.  This is the quantity that
        explain()'s gradient x input map estimates to first order, computed exactly and in closed form for every position at
        once: no second forward runs (include/vqa_hip.h vqa_occl_logit has the formulas; the classifier's first layer is
        applied to every feature row of the distinct asked images, in chunks of images that fit a 256 MiB workspace, and one
        streaming kernel does the rest).  Eval mode, the question held fixed; signed, not upsampled, not normalised.

        window: an odd int in 1..7 (default 1: single positions); anything else, a bool included, is a ValueError raised
        before any device work.

        Conditioning.  The occluded attention is renormalised by alpha = 1 / (1 - mass + |S| * r) per glimpse, where mass is
        the attention S(p) held and r the weight an occluded position keeps.  The closed form subtracts like-sized numbers and
        multiplies the difference by alpha, so its fp32 rounding error grows in proportion to alpha: the maps agree with the
        brute-force route to a few ulp of the logit while alpha <= 16, and stay defined and finite beyond that, with an error
        that grows as the window swallows the whole attention mass (DESIGN.md 4.18 records it at mass 0.99).

        answers, logits, the `answers` argument, the argument rules and the refusals are explain()'s, judged before any device
        work: eval mode only (RuntimeError in train mode), fp32 / fp32x3 (NotImplementedError for "bf16"), features that hold
        v', the feature-ownership checks and image_index rules; all three do_option values; fp32 and float16 caches (a float16
        cache gives, bit for bit, what feats.to(torch.float32) gives); a CUDA `answers` entry outside [0, A) gives a map of
        zeros; B == 0 returns empty tensors.  Rows come back in the caller's order and do not depend on how the batch is
        ordered.  Nothing is kept for a backward: _last_ctx, the gradient buffer, p.grad and the dropout seed stream are left
        alone.

        _u_bytes (tests and tools): the workspace cap in bytes, to force several chunks at small sizes."""
        door = partial(self._ask_questions, "explain_occlusion", feats, q, q_len, image_index, answers)
        return self._explain_occlusion(door, feats, window, _u_bytes)

    def _explain_occlusion(self, door, feats, window, u_bytes) -> Occlusion:
        def member(ask):
            rows, slot = self._ask_upload_asked(feats, ask)
            out = self._ask_run(self._engine.explain_occlusion, feats, ask, rows, slot, ask.own, u_bytes)
            return self._maps_result(Occlusion, feats, out)
        return self._explain_member(door, feats, Occlusion, lambda what, B: _check_window(what, window), member)

    @torch.no_grad()
    def explain_occlusion_pairs(self, feats: ImageFeatures, qfeats: QuestionFeatures, image_index, question_index,
                                answers=None, window: int = 1, *, _u_bytes=None) -> Occlusion:
        """explain_occlusion() for B (image, question) pairs from the two caches, as answer_pairs() is to answer(): pair b
        looks at image image_index[b] of `feats` with question question_index[b] of `qfeats`; no recurrence runs either.  maps,
        answers, window and the `answers` argument are explain_occlusion()'s; logits are answer_pairs()'s for the same
        arguments, bit for bit; the index rules, ownership checks and errors are answer_pairs()'s, with the window and
        `answers` checks judged first."""
        door = partial(self._ask_pairs, "explain_occlusion_pairs", feats, qfeats, image_index, question_index, answers)
        return self._explain_occlusion(door, feats, window, _u_bytes)

    # ------------------------------------------------------------------ deletion and insertion curves of an attribution map
    @torch.no_grad()
    def explain_faithfulness(self, feats: ImageFeatures, q, q_len, image_index, maps, answers=None, *,
                             _u_bytes=None) -> Faithfulness:
        """answer() with the deletion and insertion curves of a caller-supplied map per question: Faithfulness(deletion fp32
        [B, P+1], insertion fp32 [B, P+1], order int64 [B, P], answers int64 [B], logits fp32 [B, A]), P = gh * gw.  For
        question b about image n = image_index[b] and the answer column a_b = answers[b],

            order[b, :]     = the grid positions by descending maps[b, :], equal values by the smaller position
            deletion[b, k]  = logits[b, a_b] with the positions order[b, :k] absent
            insertion[b, k] = logits[b, a_b] with only the positions order[b, :k] present              k = 0 .. P

        where "absent" is explain_occlusion()'s "occluded": the rows of vn (hence of v') are zero, exactly what answer()
        computes on a cache with those rows zeroed.  deletion[:, 0] and insertion[:, P] are the full logit, deletion[:, P] and
        insertion[:, 0] the logit of the empty image (bit-equal).  This is the standard measure of how well a map RANKS the
        positions, so two maps of the same question can be compared: the better ranking has the smaller deletion_auc() and the
        larger insertion_auc().  Both whole curves cost about as much as one explain_occlusion() call: the same U product
        (the classifier's first layer on every feature row of the distinct asked images, in chunks of images under a 256 MiB
        workspace), a ranking kernel and a streaming walk along the ranking (include/vqa_hip.h vqa_rank_desc, vqa_occl_curves).
        Eval mode, the question held fixed; logit curves, not probability curves.

        maps: a floating tensor of B * P elements shaped [B, gh, gw] or [B, P], on the host or on the cache's device, used as
        fp32 -- what explain(), explain_pairs(), explain_occlusion() give as .maps, or one glimpse of answer(...,
        return_attention=True); a random map is the baseline.  Neither upsampled nor normalised: only its order matters.  -0.0
        and +0.0 are equal and NaN ranks last.  TypeError for a non-floating dtype, ValueError for a wrong element count or
        shape or for P above 8192, all raised before any device work.

        Conditioning.  Every sum runs over the positions that remain, so nothing is subtracted and the alpha <= 16 condition of
        explain_occlusion() does not apply: the curves keep their relative accuracy when a kept set holds a hundredth of the
        attention mass and alpha reaches the thousands (DESIGN.md 4.20 has the measured error).

        answers, logits, the `answers` argument, the argument rules and the refusals are explain()'s, judged before any device
        work: eval mode only (RuntimeError in train mode), fp32 / fp32x3 (NotImplementedError for "bf16"), features that hold
        v', the feature-ownership checks and image_index rules; all three do_option values; fp32 and float16 caches (a float16
        cache gives, bit for bit, what feats.to(torch.float32) gives); a CUDA `answers` entry outside [0, A) gives two rows of
        +0.0; B == 0 returns empty tensors.  Rows come back in the caller's order and do not depend on how the batch is
        ordered.  Nothing is kept for a backward: _last_ctx, the gradient buffer, p.grad and the dropout seed stream are left
        alone.

        Not offered: bf16 mode, train mode, data parallelism; strided or coarser curves; word-level and pixel-level curves;
        upsampling or normalising the maps.  Probability curves and the arg-max at every step: explain_faithfulness_probs().

        _u_bytes (tests and tools): the workspace cap in bytes, to force several chunks at small sizes."""
        door = partial(self._ask_questions, "explain_faithfulness", feats, q, q_len, image_index, answers)
        return self._explain_faithfulness(door, feats, maps, _u_bytes)

    def _explain_faithfulness(self, door, feats, maps, u_bytes) -> Faithfulness:
        def member(ask):
            rows, slot = self._ask_upload_asked(feats, ask)
            deletion, insertion, order, cols, logits = self._ask_run(self._engine.explain_faithfulness, feats, ask, rows, slot,
                                                                     self._device_maps(feats, ask, maps), u_bytes)
            return Faithfulness(deletion, insertion, order.long(), cols.long(), logits)
        own = lambda what, B: _check_maps(what, maps, B, getattr(feats, "grid", None))
        return self._explain_member(door, feats, Faithfulness, own, member)

    @torch.no_grad()
    def explain_faithfulness_pairs(self, feats: ImageFeatures, qfeats: QuestionFeatures, image_index, question_index, maps,
                                   answers=None, *, _u_bytes=None) -> Faithfulness:
        """explain_faithfulness() for B (image, question) pairs from the two caches, as answer_pairs() is to answer(): pair b
        looks at image image_index[b] of `feats` with question question_index[b] of `qfeats`; no recurrence runs either.  The
        curves, order, answers, maps and the `answers` argument are explain_faithfulness()'s; logits are answer_pairs()'s for the
        same arguments, bit for bit; the index rules, ownership checks and errors are answer_pairs()'s, with the maps and
        `answers` checks judged first."""
        door = partial(self._ask_pairs, "explain_faithfulness_pairs", feats, qfeats, image_index, question_index, answers)
        return self._explain_faithfulness(door, feats, maps, _u_bytes)

    # ------------------------------------------------------------------ probability curves and flip points
    @torch.no_grad()
    def explain_faithfulness_probs(self, feats: ImageFeatures, q, q_len, image_index, maps, answers=None, *, _u_bytes=None,
                                   _ws_bytes=None) -> ProbabilityCurves:
        """explain_faithfulness() on probabilities, with the arg-max at every step: ProbabilityCurves(deletion, insertion fp32
        [B, P+1], deletion_top, insertion_top int32 [B, P+1], deletion_top_prob, insertion_top_prob fp32 [B, P+1], order int64
        [B, P], answers int64 [B], logits fp32 [B, A]), P = gh * gw.  With order and "absent" as explain_faithfulness() has
        them, and logits_K the logits answer() computes on a cache that holds only the rows of the kept set K,

            deletion[b, k]      = softmax(logits_K)[a_b]               K = order[b, k:]
            insertion[b, k]     = the same                             K = order[b, :k]                  k = 0 .. P
            deletion_top[b, k]  = the arg-max column of logits_K, ties by the smaller column (topk_answers' order)
            deletion_top_prob   = its probability; insertion_top and insertion_top_prob likewise

        deletion[:, 0] and insertion[:, P] are softmax(logits)[b, a_b]; deletion[:, P] and insertion[:, 0] belong to the empty
        image (bit-equal).  deletion_auc() and insertion_auc() are the deletion / insertion metric as it is published, on the
        class probability: unlike explain_faithfulness()'s logit curves they do not move when a constant is added to every
        logit.  deletion_flip() is the number of the map's best positions that must go before the answer changes,
        insertion_flip() how few of them get it back (P + 1: never).

        How it runs.  The brute-force route is answer() on 2 (P + 1) edited banks per question, then torch.softmax.  Here
        explain_faithfulness()'s parts run as they are (the base run, the ranking, the U product per chunk of images), the walk
        along the ranking keeps each kept set's hidden row instead of one column's dot product (include/vqa_hip.h
        vqa_occl_curves_hidden), one product with lin2 -- plain fp32 in every compute mode -- gives every column of every step,
        and one kernel reads each logits row once (vqa_softmax_pick).  The questions of a chunk of images go through in
        sub-chunks of whole questions whose curve workspace, hidden rows and logits stay within 256 MiB.

        maps, answers, logits, order, the `answers` argument, the argument rules and the refusals are explain_faithfulness()'s,
        judged before any device work; logits are answer()'s and order is explain_faithfulness()'s, bit for bit.  A CUDA
        `answers` entry outside [0, A) gives two probability rows of +0.0; the tops do not depend on the column.  A float16
        cache gives, bit for bit, what feats.to(torch.float32) gives; B == 0 returns empty tensors.  Rows come back in the
        caller's order; how the batch is ordered and chunked may move the lin2 product's tiles, hence the last bits.

        Not offered: probability-valued Shapley or occlusion maps, strided curves, word- and pixel-level curves, bf16 mode,
        train mode, data parallelism.

        _u_bytes, _ws_bytes (tests and tools): the two workspace caps in bytes, to force several chunks at small sizes."""
        door = partial(self._ask_questions, "explain_faithfulness_probs", feats, q, q_len, image_index, answers)
        return self._explain_faithfulness_probs(door, feats, maps, _u_bytes, _ws_bytes)

    def _explain_faithfulness_probs(self, door, feats, maps, u_bytes, ws_bytes) -> ProbabilityCurves:
        def member(ask):
            rows, slot, by_slot = self._ask_upload_asked(feats, ask, grouped=True)
            prob, top, top_prob, order, cols, logits = self._ask_run(
                self._engine.explain_faithfulness_probs, feats, ask, rows, slot, by_slot, ask.offsets,
                self._device_maps(feats, ask, maps), u_bytes, ws_bytes)
            return ProbabilityCurves(prob[:, 0], prob[:, 1], top[:, 0], top[:, 1], top_prob[:, 0], top_prob[:, 1], order.long(),
                                     cols.long(), logits)
        own = lambda what, B: _check_maps(what, maps, B, getattr(feats, "grid", None))
        return self._explain_member(door, feats, ProbabilityCurves, own, member)

    @torch.no_grad()
    def explain_faithfulness_probs_pairs(self, feats: ImageFeatures, qfeats: QuestionFeatures, image_index, question_index, maps,
                                         answers=None, *, _u_bytes=None, _ws_bytes=None) -> ProbabilityCurves:
        """explain_faithfulness_probs() for B (image, question) pairs from the two caches, as answer_pairs() is to answer():
        pair b looks at image image_index[b] of `feats` with question question_index[b] of `qfeats`; no recurrence runs either.
        The curves, tops, order, answers, maps and the `answers` argument are explain_faithfulness_probs()'s; logits are
        answer_pairs()'s for the same arguments, bit for bit; the index rules, ownership checks and errors are answer_pairs()'s,
        with the maps and `answers` checks judged first."""
        door = partial(self._ask_pairs, "explain_faithfulness_probs_pairs", feats, qfeats, image_index, question_index, answers)
        return self._explain_faithfulness_probs(door, feats, maps, _u_bytes, _ws_bytes)

    # ------------------------------------------------------------------ sampled Shapley maps from cached features
    @torch.no_grad()
    def explain_shapley(self, feats: ImageFeatures, q, q_len, image_index, answers=None, permutations: int = 16, *, seed: int = 0,
                        orders=None, _u_bytes=None, _ws_bytes=None) -> Shapley:
        """answer() with a sampled Shapley map per question: Shapley(maps fp32 [B, gh, gw], stderr fp32 [B, gh, gw], answers
        int64 [B], logits fp32 [B, A], baseline_logits fp32 [B]).  For question b about image n = image_index[b] and the answer
        column a_b = answers[b], let f_b(S) be logits[b, a_b] with only the grid positions S present -- "absent" is
        explain_occlusion()'s "occluded": the rows of vn (hence of v') are zero; eval mode, the question held fixed.  The Shapley
        value of position p is its marginal contribution f_b(S + p) - f_b(S) averaged over the sets S that precede p in a
        uniformly random order of the positions.  explain_occlusion() asks that question for one context only (everything else
        present) and misses redundancy: two positions that each suffice both get about 0.  Here, for M drawn orders,

            e_m[b, orders[m, k]] = ((ins_m[k+1] - ins_m[k]) + (del_m[k] - del_m[k+1])) / 2              k = 0 .. P-1
            maps[b, p]           = mean over m of e_m[b, p]
            stderr[b, p]         = sqrt(sum_m (e_m[b, p] - maps[b, p])^2 / (M (M - 1))),  NaN for M = 1

        with ins_m, del_m explain_faithfulness()'s insertion and deletion curves of question b along orders[m]: the insertion
        step is the marginal of orders[m, k] under orders[m], the deletion step its marginal under the REVERSED order (the
        deletion curve read backwards is the reversed order's insertion curve), so one walk serves a permutation and its
        antithetic partner.  Every e_m telescopes, so the maps sum to logits[b, a_b] - baseline_logits[b] up to fp32 rounding
        whatever M is (completeness_gap()); baseline_logits is the logit of the empty image, explain_faithfulness()'s
        insertion[:, 0] for the same ask, bit for bit.

        permutations: an even int in 2..256 (default 16), counted WITH the reverses: permutations // 2 orders are drawn, by
        shapley_orders(permutations, P, seed) on the host (torch.randperm under a CPU generator of its own; the global seed
        stream is not touched).  A bool or another type is a TypeError, an odd or out-of-range value a ValueError.  orders: an
        integer tensor [M, P], 1 <= M <= 128, every row a permutation of 0 .. P-1, in place of permutations / seed (the
        permutations are then the 2M rows and reverses); TypeError for a non-integer dtype, ValueError for another shape or a
        row that is no permutation.  All of it is judged on the host before any device work.

        ONE table of orders is shared by every question of the call.  Each question's estimate stays unbiased; only the errors
        of different questions become correlated (do not average stderr over questions as if they were independent).  Sharing
        is what makes a row depend on its question and the table alone: rows come back in the caller's order and do not depend
        on how the batch is ordered, split or chunked, bit for bit.

        How it runs.  Composing it from explain_faithfulness() repeats the base run and the U product per order.  Here they run
        once; the curve kernels walk the (question, order) pairs from the shared table (include/vqa_hip.h
        vqa_occl_curves_orders), the orders in groups whose curve workspace stays within 256 MiB, and one kernel folds each
        group's curves into the running mean and M2 of every entry in ascending m (vqa_shapley_accumulate): the bits do not
        depend on the grouping.  No ranking runs, nothing is kept.

        answers, logits, the `answers` argument, the argument rules and the refusals are explain()'s, judged before any device
        work: eval mode only (RuntimeError in train mode), fp32 / fp32x3 (NotImplementedError for "bf16"), features that hold
        v', the feature-ownership checks and image_index rules; all three do_option values; fp32 and float16 caches (a float16
        cache gives, bit for bit, what feats.to(torch.float32) gives); a CUDA `answers` entry outside [0, A) gives a map, an
        error and a baseline of +0.0; B == 0 returns empty tensors.  Nothing is kept for a backward: _last_ctx, the gradient
        buffer, p.grad and the dropout seed stream are left alone.

        Not offered: per-question orders; other value functions (probabilities); KernelSHAP regression; Shapley values of the
        words or the pixels; bf16 mode, train mode, data parallelism.

        _u_bytes, _ws_bytes (tests and tools): the caps of U and of the curve workspace in bytes, to force several chunks and
        several groups of orders at small sizes."""
        door = partial(self._ask_questions, "explain_shapley", feats, q, q_len, image_index, answers)
        return self._explain_shapley(door, feats, permutations, seed, orders, _u_bytes, _ws_bytes)

    @staticmethod
    def _shapley_table(what: str, feats, permutations, seed, orders):
        """The host checks of permutations / seed / orders in the name `what`; returns the given table, or the function of P
        that draws it."""
        if orders is not None:
            return _check_orders(what, orders, getattr(feats, "grid", None))
        _check_permutations(what, permutations)
        if isinstance(seed, bool) or not isinstance(seed, int):
            raise TypeError(f"{what}: seed must be an int, got {type(seed).__name__}")
        return lambda P: shapley_orders(permutations, P, seed)

    def _explain_shapley(self, door, feats, permutations, seed, orders, u_bytes, ws_bytes) -> Shapley:
        def member(ask):
            P = feats.grid[0] * feats.grid[1]
            table = ask.own(P) if callable(ask.own) else ask.own
            rank = torch.empty_like(table)
            rank.scatter_(1, table, torch.arange(P).expand_as(table))        # the inverse of every row
            rows, slot, table, rank = self._ask_upload_asked(feats, ask, (table.reshape(-1), rank.reshape(-1)))
            maps, err, cols, logits, base = self._ask_run(self._engine.explain_shapley, feats, ask, rows, slot, table.view(-1, P),
                                                          rank.view(-1, P), u_bytes, ws_bytes)
            return Shapley(maps.view(-1, *feats.grid), err.view(-1, *feats.grid), cols.long(), logits, base)
        own = lambda what, B: self._shapley_table(what, feats, permutations, seed, orders)
        return self._explain_member(door, feats, Shapley, own, member)

    @torch.no_grad()
    def explain_shapley_pairs(self, feats: ImageFeatures, qfeats: QuestionFeatures, image_index, question_index, answers=None,
                              permutations: int = 16, *, seed: int = 0, orders=None, _u_bytes=None, _ws_bytes=None) -> Shapley:
        """explain_shapley() for B (image, question) pairs from the two caches, as answer_pairs() is to answer(): pair b looks
        at image image_index[b] of `feats` with question question_index[b] of `qfeats`; no recurrence runs either.  maps, stderr,
        answers, baseline_logits, permutations, seed, orders and the `answers` argument are explain_shapley()'s; logits are
        answer_pairs()'s for the same arguments, bit for bit; the index rules, ownership checks and errors are answer_pairs()'s,
        with the permutations / orders and `answers` checks judged first."""
        door = partial(self._ask_pairs, "explain_shapley_pairs", feats, qfeats, image_index, question_index, answers)
        return self._explain_shapley(door, feats, permutations, seed, orders, _u_bytes, _ws_bytes)

    # ------------------------------------------------------------------ gradient x input per question token
    @torch.no_grad()
    def explain_words(self, feats: ImageFeatures, q, q_len, image_index, answers=None, *, _stages=None) -> WordAttribution:
        """explain() carried on to the other input of the answer: WordAttribution(words fp32 [B, T], maps fp32 [B, gh, gw],
        answers int64 [B], logits fp32 [B, A]).  For question b, token slot t and the answer column a_b = answers[b], with
        e[b, t, :] = embedding.weight[q[b, t]] the embedding output before tanh,

            words[b, t] = sum_e e[b, t, e] * d logits[b, a_b] / d e[b, t, e]

        in eval mode WITH THE IMAGE FEATURES HELD FIXED: signed, not normalised.  The gradient follows the question along
        both of its paths to the logit -- the question half of the classifier input, and q' = q_lin(qf) in the attention
        scores -- back through the LSTM to the embedding stage.  For do_option '|' the second path is identically zero (the q'
        half adds the same constant to every position's score, and softmax is shift-invariant), and nothing runs for it.
        words[b, t] is 0 for t >= q_len[b], and 0 for a token id outside the vocabulary (counted as answer() counts it);
        the padding row of the embedding is zero, so a token 0 inside a question gives 0 too.  Data gradients only: no
        weight, bias or embedding gradient is formed (include/vqa_hip.h has the formulas).

        maps, answers and logits are explain()'s for the same arguments, bit for bit, and so are the `answers` argument, the
        argument rules and the refusals, all judged before any device work: eval mode only (RuntimeError in train mode),
        fp32 / fp32x3 (NotImplementedError for "bf16"), features that hold v', the feature-ownership checks and image_index
        rules; fp32 and float16 caches (a float16 cache gives, bit for bit, what feats.to(torch.float32) gives); B == 0
        returns empty tensors.  Nothing is kept for a backward: _last_ctx, the gradient buffer, p.grad and the dropout seed
        stream are left alone, and a later forward / backward is unchanged.

        There is no explain_words_pairs: QuestionFeatures holds the encoder's results (qf, q'), not the recurrence state
        (gates, hidden and cell states per step) that the gradient has to go back through, so cached questions cannot be
        explained without encoding them again -- which is this call.

        _stages (tests and tools): a dict that receives the engine's intermediate gradients (Engine.explain_words)."""
        def member(ask):
            self._ask_upload(feats, ask)
            words, maps, cols, logits = self._ask_run(self._engine.explain_words, feats, ask, _stages)
            return WordAttribution(words, maps.view(-1, *feats.grid), cols.long(), logits)
        door = partial(self._ask_questions, "explain_words", feats, q, q_len, image_index, answers, host_first=True)
        return self._explain_member(door, feats, WordAttribution, None, member)

    # ------------------------------------------------------------------ exact word occlusion from cached features
    _WORD_TABLE_FIELDS = ("fwd_b", "fwd_t", "fwd_seed", "rev_b", "rev_t", "rev_seed", "rev_row", "order", "offsets", "img")

    @torch.no_grad()
    def explain_words_occlusion(self, feats: ImageFeatures, q, q_len, image_index, answers=None, *,
                                _variant_rows=None) -> WordOcclusion:
        """answer() with the exact occlusion value of every question token: WordOcclusion(words fp32 [B, T], answers int64 [B],
        logits fp32 [B, A]).  For question b, token slot t < q_len[b] and the answer column a_b = answers[b], with e[b, t, :] =
        embedding.weight[q[b, t]] the embedding output before tanh,

            words[b, t] = logits[b, a_b] - logit_t[b, a_b]

        where logit_t is the same forward with e[b, t, :] replaced by the zero vector, in eval mode WITH THE IMAGE FEATURES HELD
        FIXED: the LSTM input of that step is tanh(0) = 0, so its gate pre-activation is b_ih + b_hh + h W_hh^T; the question's
        length and every other token are unchanged.  This is the quantity whose first-order estimate is explain_words().words --
        occluding a word means zeroing its input, as explain_occlusion() zeroes feature rows -- and through an LSTM that
        estimate is a poor one (DESIGN.md 4.19 records how far apart they are).  It is defined on the embedding output, so it does
        not depend on what row 0 of the table holds.  Signed, not normalised.

        words[b, t] is +0.0 for t >= q_len[b], and a row is all zeros where answers[b] is outside [0, A) (a CUDA `answers`
        entry, as explain()'s map).  A slot whose embedding row is zero already -- token 0, and an id outside the vocabulary,
        which the forward reads as a zero row and counts -- is NOT forced to zero: its value is the difference of two evaluations
        of the same function along two kernel routes (the base run's recurrence and the variant steps), a few ulp of the
        logit, within the parity bound of the tests.

        How it runs.  The recurrence has no closed form, but it has shared prefixes: zeroing slot t leaves the forward
        direction's state before t and the reverse direction's state after t as answer()'s own encoder run left them.  A
        variant (b, t) therefore takes q_len[b] - t forward and t + 1 reverse steps from those saved states instead of 2 *
        q_len[b], and its tail needs one column of lin2, not A (include/vqa_hip.h vqa_lstm_occl_cell_fwd, vqa_occl_words).
        The variant table is built on the host from the lengths: device-resident lengths are copied to the host ONCE, which
        synchronises (as a CUDA image_index does).  The questions are walked in chunks whose variant buffers stay within a 256
        MiB workspace; chunks cut between questions.

        answers and logits are explain()'s for the same arguments, bit for bit, and so are the `answers` argument, the argument
        rules and the refusals, all judged before any device work: eval mode only (RuntimeError in train mode), fp32 / fp32x3
        (NotImplementedError for "bf16"), features that hold v', the feature-ownership checks and image_index rules; fp32 and
        float16 caches (a float16 cache gives, bit for bit, what feats.to(torch.float32) gives); B == 0 returns empty tensors.
        Nothing is kept for a backward: _last_ctx, the gradient buffer, p.grad and the dropout seed stream are left alone, and a
        later forward / backward is unchanged.

        There is no pairs form, for the reason explain_words() gives: QuestionFeatures holds the encoder's results, not the
        per-step states the variant chains start from.

        _variant_rows (tests and tools): caps the variants per chunk, to force several chunks at small sizes."""
        def member(ask):
            T = ask.q.shape[1]
            lengths = ask.q_len.detach().to(device="cpu", dtype=torch.int64).reshape(-1)  # the one copy to the host: synchronises
            cap = self._engine.word_occlusion_rows(feats.vn.shape[1])
            if _variant_rows is not None:
                cap = max(1, min(cap, int(_variant_rows)))
            img, fields = ask.index[2], self._WORD_TABLE_FIELDS
            chunks = []
            for b0, b1 in word_occlusion_chunks(lengths.tolist(), T, cap):
                tab = word_occlusion_table(lengths, T, b0, b1)
                tab.img = img[tab.fwd_b.long()]
                tab.order, tab.offsets = _group(tab.img, feats.N)
                chunks.append(tab)
            on_device = self._ask_upload(feats, ask, [getattr(tab, k) for tab in chunks for k in fields])
            for i, tab in enumerate(chunks):                                            # the tables on the device: the same copy
                vars(tab).update(zip(fields, on_device[i * len(fields):]))
            words, picked, logits = self._ask_run(self._engine.explain_words_occlusion, feats, ask, chunks)
            return WordOcclusion(words, picked.long(), logits)
        door = partial(self._ask_questions, "explain_words_occlusion", feats, q, q_len, image_index, answers, host_first=True)
        return self._explain_member(door, feats, WordOcclusion, None, member)
