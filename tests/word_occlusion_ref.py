"""float64 references for the exact word occlusion of VqaNet.explain_words_occlusion (include/vqa_hip.h):

  brute                the definition, by brute force: one full forward per (b, t) with the embedding output e[b, t, :] = 0,
                       through the oracle's pieces as word_attribution_ref.autograd_reference goes through them
                       (question_features, attention_scores, image_question_attention, classifier);
  cell_step            one step of the variant cell (the header's formula of vqa_lstm_occl_cell_fwd), restated;
  prefix_shared        the same words from prefix-shared chains: the base run's states per slot, then for every variant only
                       the remaining steps, by the host table (dl_vqa_amd.model.word_occlusion_table) and cell_step -- the schedule
                       the engine runs, in float64;
  tail                 the header's formula of vqa_occl_words, restated;
  first_order          explain_words' float64 words (gradient x input) for the same arguments;
  fixture_brute        brute for the pairs tests/attribution_ref.py asks of a golden fixture, computed once per columns.

Everything here runs on the CPU; the GPU tests import it and compute each reference once."""
import functools

import torch
import torch.nn.functional as F

from tests import attribution_ref as R
from tests import word_attribution_ref as W
from tests.explain_util import columns        # noqa: F401 -- the given answer columns, under the name the tests ask for

_SFX = W._SFX


def case_sd(case):
    return case["sd"] if "sd" in case else case["golden"].sd


def _logits(sd, do_option, vn, x, q_len, img, grid, bidirectional):
    """Eval-mode logits [rows, A] from x = tanh(e) [rows, T, E]."""
    qf = W.question_features(sd, x, q_len, bidirectional)
    return R.forward64(sd, do_option, vn, qf, img, grid)


def variants(q_len, T):
    """The pairs (b, t), t < min(q_len[b], T), b-major."""
    return [(b, t) for b, n in enumerate(q_len.tolist()) for t in range(min(max(int(n), 0), T))]


def brute(sd, do_option, vn, q, q_len, img, answers, grid, bidirectional):
    """words [B, T] by the definition: the logit of column answers[b] minus the same logit of a full forward whose embedding
    output at slot t is the zero vector; 0 for t >= q_len[b]."""
    sd = R._sd64(sd)
    img = torch.as_tensor(img, dtype=torch.int64)
    cols = torch.as_tensor(answers, dtype=torch.int64)
    B, T = q.shape
    e = F.embedding(q, sd["text.embedding.weight"])
    base = _logits(sd, do_option, vn, torch.tanh(e), q_len, img, grid, bidirectional)
    pairs = variants(q_len, T)
    vb = torch.tensor([b for b, _ in pairs], dtype=torch.int64)
    ev = e[vb].clone()
    for r, (_, t) in enumerate(pairs):
        ev[r, t] = 0
    occluded = _logits(sd, do_option, vn, torch.tanh(ev), q_len[vb], img[vb], grid, bidirectional)
    words = torch.zeros(B, T, dtype=torch.float64)
    for r, (b, t) in enumerate(pairs):
        words[b, t] = base[b, cols[b]] - occluded[r, cols[b]]
    return words, base


def cell_step(xg_base, xg0, hg, h, c, q_len, var_b, var_t, s):
    """One step, time s, of n variant rows in float64: row r = (var_b[r], var_t[r]) is held for s >= q_len[b]; otherwise pre =
    (xg0 if s == t else xg_base[s, b]) + hg[r], gate order i, f, g, o, c = sig(f) c + sig(i) tanh(g), h = sig(o) tanh(c).
    xg_base [T, B, 4H], xg0 [4H], hg [n, 4H], h and c [n, H].  Returns the new (h, c)."""
    xg_base, xg0, hg, h, c = (t.double() for t in (xg_base, xg0, hg, h, c))
    b, t = var_b.long(), var_t.long()
    H = h.shape[1]
    pre = torch.where((t == s)[:, None], xg0[None, :].expand(len(b), -1), xg_base[s, b]) + hg
    i, f, g, o = pre.split(H, dim=1)
    c_new = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
    h_new = torch.sigmoid(o) * torch.tanh(c_new)
    active = (q_len.long()[b] > s)[:, None]
    return torch.where(active, h_new, h), torch.where(active, c_new, c)


def base_states(x, q_len, w_ih, w_hh, b_ih, b_hh, reverse):
    """The base run of one direction in the engine's layout: xg [T, B, 4H] (both biases in), Hs and Cs [T + 1, B, H] -- the
    forward direction reads slot t and writes t + 1, the reverse reads t + 1 and writes t; finished samples hold."""
    B, T, _ = x.shape
    H = w_hh.shape[1]
    xg = (x @ w_ih.t() + b_ih + b_hh).permute(1, 0, 2).contiguous()
    Hs, Cs = x.new_zeros(T + 1, B, H), x.new_zeros(T + 1, B, H)
    every_b, never = torch.arange(B), torch.full((B,), -1)
    for s in (range(T - 1, -1, -1) if reverse else range(T)):
        si, so = (s + 1, s) if reverse else (s, s + 1)
        Hs[so], Cs[so] = cell_step(xg, xg[0, 0], Hs[si] @ w_hh.t(), Hs[si], Cs[si], q_len, every_b, never, s)
    return xg, Hs, Cs


def prefix_shared(sd, do_option, vn, q, q_len, img, answers, grid, bidirectional, chunk_rows=None):
    """brute's words from prefix-shared chains, by the host table and cell_step; also returns the row-steps of the recurrent
    products that were run."""
    from dl_vqa_amd.model import word_occlusion_chunks, word_occlusion_table
    sd = R._sd64(sd)
    img = torch.as_tensor(img, dtype=torch.int64)
    cols = torch.as_tensor(answers, dtype=torch.int64)
    B, T = q.shape
    x = torch.tanh(F.embedding(q, sd["text.embedding.weight"]))
    base = _logits(sd, do_option, vn, x, q_len, img, grid, bidirectional)
    dirs = []
    for d in range(2 if bidirectional else 1):
        w = [sd[f"text.lstm.{k}_l0" + _SFX[d]] for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
        dirs.append((w, base_states(x, q_len, *w, bool(d))))
    words = torch.zeros(B, T, dtype=torch.float64)
    row_steps = 0
    for b0, b1 in word_occlusion_chunks(q_len.tolist(), T, chunk_rows):
        tab = word_occlusion_table(q_len, T, b0, b1)
        if tab.V == 0:
            continue
        H = dirs[0][0][1].shape[1]
        qf = torch.zeros(tab.V, len(dirs) * H, dtype=torch.float64)
        for d, ((w_ih, w_hh, b_ih, b_hh), (xg, Hs, Cs)) in enumerate(dirs):
            var_b, var_t, seed = (tab.rev_b, tab.rev_t, tab.rev_seed) if d else (tab.fwd_b, tab.fwd_t, tab.fwd_seed)
            counts = tab.n_rev if d else tab.n_fwd
            h, c = Hs.reshape(-1, H)[seed.long()].clone(), Cs.reshape(-1, H)[seed.long()].clone()
            for s in (range(tab.steps - 1, -1, -1) if d else range(tab.steps)):
                n = counts[s]
                if n == 0:
                    continue
                row_steps += n
                h[:n], c[:n] = cell_step(xg, b_ih + b_hh, h[:n] @ w_hh.t(), h[:n], c[:n], q_len, var_b[:n], var_t[:n], s)
            rows = tab.rev_row.long() if d else torch.arange(tab.V)
            qf[rows, d * H:(d + 1) * H] = c
        vb, vt = tab.fwd_b.long(), tab.fwd_t.long()
        occluded = R.forward64(sd, do_option, vn, qf, img[vb], grid)
        words[vb, vt] = base[vb, cols[vb]] - occluded[torch.arange(tab.V), cols[vb]]
    return words, row_steps


def tail(h1, W2, b2, answers, logits, var_b, var_t, q_len, B, T):
    """vqa_occl_words in float64: [B, T]; a column outside [0, A) gives a zero row, slots that are no variant 0."""
    h1, W2, b2, logits = (t.double() for t in (h1, W2, b2, logits))
    A = W2.shape[0]
    out = torch.zeros(B, T, dtype=torch.float64)
    for r, (b, t) in enumerate(zip(var_b.tolist(), var_t.tolist())):
        a = int(answers[b])
        if 0 <= a < A and t < int(q_len[b]):
            out[b, t] = logits[b, a] - (W2[a] @ h1[r] + b2[a])
    return out


def first_order(case, do_option, answers):
    """explain_words' float64 words for the same arguments."""
    return W.autograd_reference(case_sd(case), do_option, case["vn"], case["q"], case["q_len"], case["img"], list(answers),
                                case["grid"], case["cfg"]["text"]["bidirectional"])["words"]


def case_brute(case, do_option, answers):
    return brute(case_sd(case), do_option, case["vn"], case["q"], case["q_len"], case["img"], list(answers), case["grid"],
                 case["cfg"]["text"]["bidirectional"])[0]


@functools.lru_cache(maxsize=None)
def _fixture_brute(do_option, answers):
    return case_brute(R.fixture_case(do_option), do_option, answers)


def fixture_brute(do_option, answers):
    """brute's words for the fixture's pairs and the given answer columns, computed once per (fixture, columns)."""
    return _fixture_brute(do_option, tuple(int(a) for a in answers))


