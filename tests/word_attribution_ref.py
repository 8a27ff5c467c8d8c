"""float64 references for the per-token gradient x input of VqaNet.explain_words (include/vqa_hip.h):

  autograd_reference   words [B, T] = (e * d logit[b, a_b] / d e).sum(-1) by torch.autograd through the oracle's pieces
                       (lstm_direction, attention_scores, image_question_attention, classifier), with the embedding output
                       e = F.embedding(q, emb) as the leaf and the image features vn[img] as constants.  It also returns the
                       gradients at x = tanh(e), at q' and at the question features.  part = "attention" detaches the
                       classifier's question input, part = "classifier" the attention's: the two paths of the question.
  dq_closed_form       step 3 of the chain, the header's formula of vqa_att_attr_dq_grouped, from dscore;
  words_closed_form    step 7, the header's formula of vqa_embed_attr, from the gradient at x;
  fixture_reference    the above for the pairs tests/attribution_ref.py asks of a golden fixture, computed once;
  random_case          a seeded random model from tiny_cfg with H = 32 (the fused recurrence), its features and questions.

Everything here runs on the CPU; the GPU tests import it and compute each reference once."""
import functools

import torch
import torch.nn.functional as F

from oracle import vqa_oracle as O
from tests import attribution_ref as R

_SFX = ("", "_reverse")


def question_features(sd, x, q_len, bidirectional):
    """[c_fwd | c_bwd] [B, Q] from x = tanh(e) [B, T, E], by oracle.lstm_direction per direction."""
    cs = []
    for d in range(2 if bidirectional else 1):
        _, c = O.lstm_direction(x, q_len, sd["text.lstm.weight_ih_l0" + _SFX[d]], sd["text.lstm.weight_hh_l0" + _SFX[d]],
                                sd["text.lstm.bias_ih_l0" + _SFX[d]], sd["text.lstm.bias_hh_l0" + _SFX[d]], bool(d))
        cs.append(c)
    return torch.cat(cs, dim=1)


def autograd_reference(sd, do_option, vn, q, q_len, img, answers, grid, bidirectional, part="full", dtype=torch.float64):
    """A dict: words [B, T], e, x [B, T, E], qf [B, Q], qp [B, mid] and the gradients of sum_b logit[b, a_b] at them (de, dx,
    dqf, dqp; zeros where `part` cuts the path), logits [B, A].  vn [N, P, C]; img, answers: lists or tensors.
    dtype float32 evaluates the same graph in fp32 (how far a faithful fp32 evaluation is from float64)."""
    assert part in ("full", "attention", "classifier")
    sd = {k: (t.to(dtype) if t.is_floating_point() else t) for k, t in sd.items()}
    img = torch.as_tensor(img, dtype=torch.int64)
    e = F.embedding(q, sd["text.embedding.weight"]).detach().requires_grad_(True)
    x = torch.tanh(e)
    qf = question_features(sd, x, q_len, bidirectional)
    q_att = qf.detach() if part == "classifier" else qf
    q_cls = qf.detach() if part == "attention" else qf
    # q' as a tensor of this graph: the oracle's attention_scores applies q_lin itself, so it is handed q' and an identity
    # q_lin (x . I^T + 0 is exact)
    qp = F.linear(q_att, sd["attention.q_lin.weight"], sd["attention.q_lin.bias"])
    mid = qp.shape[1]
    sd_id = dict(sd)
    sd_id["attention.q_lin.weight"] = torch.eye(mid, dtype=dtype)
    sd_id["attention.q_lin.bias"] = torch.zeros(mid, dtype=dtype)
    v = R._as_maps(vn.to(dtype)[img], grid)
    att = O.attention_scores(sd_id, v, qp, do_option)
    wv, _ = O.image_question_attention(v, att)
    logits = O.classifier(sd, torch.cat([wv, q_cls], dim=1))
    picked = logits.gather(1, torch.as_tensor(answers, dtype=torch.int64)[:, None]).sum()
    wanted = [t for t in (e, x, qf, qp) if t.requires_grad]
    grads = dict(zip((id(t) for t in wanted), torch.autograd.grad(picked, wanted, allow_unused=True)))
    g = lambda t: grads.get(id(t)) if grads.get(id(t)) is not None else torch.zeros_like(t)
    de = g(e)
    return {"words": (e.detach() * de).sum(-1), "e": e.detach(), "x": x.detach(), "qf": qf.detach(), "qp": qp.detach(), "de": de,
            "dx": g(x), "dqf": g(qf), "dqp": g(qp), "logits": logits.detach()}


def dq_closed_form(dscore, vp, qp, wx, img, mode):
    """Step 3: dq_att [B, mid] = sum_p dxpre ('+') or sum_p dxpre * v' ('*'), dxpre = [x > 0] * sum_g dscore * wx[g]; zeros for
    '|' (the q' half shifts every position's score by the same constant).  dscore [B, G, P], vp [N, P, mid], qp [B, mid]."""
    dscore, vp, qp, wx = (t.double() for t in (dscore, vp, qp, wx))
    if mode == 2:
        return torch.zeros_like(qp)
    mid = vp.shape[-1]
    v, q = vp[torch.as_tensor(img, dtype=torch.int64)], qp[:, None, :]
    pre = v + q if mode == 0 else v * q
    dxpre = (pre > 0).double() * torch.einsum("bgp,gm->bpm", dscore, wx[:, :mid])
    return dxpre.sum(1) if mode == 0 else (dxpre * v).sum(1)


def words_closed_form(emb, q, x, dx, q_len):
    """Step 7: words [B, T] = sum_e emb[q] * (1 - x^2) * dx, 0 for t >= q_len[b] and for a token id outside [0, V).
    x, dx [B, T, E] (batch-major here)."""
    emb, x, dx = emb.double(), x.double(), dx.double()
    V = emb.shape[0]
    ok = (q >= 0) & (q < V)
    w = (emb[q.clamp(0, V - 1)] * (1 - x * x) * dx).sum(-1)
    T = q.shape[1]
    live = torch.arange(T)[None, :] < q_len[:, None]
    return torch.where(ok & live, w, torch.zeros_like(w))


def reference_parts(sd, do_option, vn, q, q_len, img, answers, grid, bidirectional):
    """(full, attention-only, classifier-only) autograd_reference dicts."""
    return tuple(autograd_reference(sd, do_option, vn, q, q_len, img, answers, grid, bidirectional, part)
                 for part in ("full", "attention", "classifier"))


@functools.lru_cache(maxsize=None)
def _fixture_reference(do_option, answers):
    f = R.fixture_case(do_option)
    return reference_parts(f["golden"].sd, do_option, f["vn"], f["q"], f["q_len"], f["img"], list(answers), f["grid"],
                           f["cfg"]["text"]["bidirectional"])


def fixture_reference(do_option, answers):
    """(full, attention-only, classifier-only) for the fixture's pairs and the given answer columns, computed once per
    (fixture, columns) and shared by the tests that need it."""
    return _fixture_reference(do_option, tuple(int(a) for a in answers))


def fixture_argmax(do_option):
    """The arg-max answer columns of the fixture's pairs in float64 (ties by the smaller column)."""
    f = R.fixture_case(do_option)
    logits = R.forward64(f["golden"].sd, do_option, f["vn"], f["qf"], f["img"], f["grid"])
    return [int(a) for a in logits.argmax(1)]


# ----------------------------------------------------------------------------- a random model on the fused recurrence
RANDOM_SEED = 5            # chosen on the CPU so that near_zero_count is 0 for both encoders (asserted by the tests)
RANDOM_IMAGE_INDEX = (0, 2, 1, 1, 0)
RANDOM_Q_LEN = (6, 1, 4, 6, 3)


@functools.lru_cache(maxsize=None)
def random_case(bidirectional, T=6, seed=RANDOM_SEED):
    """A seeded random model from tiny_cfg with question_features = 32 (H % 32 == 0: the fused recurrence), B = 5 questions of
    T slots with ragged lengths including 1 and T, about 3 images.  A dict as attribution_ref.fixture_case's, plus sd, V."""
    from dl_vqa_amd import VqaNet
    from tests.golden_util import Golden, tiny_cfg
    g = Golden("tiny_plus")
    cfg = tiny_cfg(g.meta)
    cfg["text"] = dict(cfg["text"], question_features=32, bidirectional=bool(bidirectional))
    V = g.meta["V"]
    torch.manual_seed(seed)
    sd = {k: t.detach().clone() for k, t in VqaNet(cfg, V).state_dict().items()}
    gen = torch.Generator().manual_seed(seed + 1)
    B = len(RANDOM_IMAGE_INDEX)
    q_len = torch.tensor(RANDOM_Q_LEN).clamp(max=T)
    q = torch.randint(1, V, (B, T), generator=gen)
    q = torch.where(torch.arange(T)[None, :] < q_len[:, None], q, torch.zeros_like(q))
    v = g.t["v"][:3]
    sd64 = R._sd64(sd)
    xi = O.l2_normalise(O.image_encoder(sd64, v.double(), cfg["image"]["stride"]))
    grid = tuple(xi.shape[2:])
    vn = xi.reshape(xi.shape[0], xi.shape[1], -1).permute(0, 2, 1).contiguous()
    qf = O.question_encoder(sd64, q, q_len, bool(bidirectional))
    return {"cfg": cfg, "sd": sd, "V": V, "v": v, "q": q, "q_len": q_len, "img": torch.tensor(RANDOM_IMAGE_INDEX), "vn": vn,
            "qf": qf, "grid": grid}


def case_near_zero(case, do_option):
    """attribution_ref.near_zero_count of a case (fixture_case or random_case) and of its classifier's hidden layer: the ReLU
    pre-activations whose indicator an fp32 evaluation may put on the other side."""
    sd = case["sd"] if "sd" in case else case["golden"].sd
    args = R.model_inputs(sd, do_option, case["vn"], case["qf"], case["img"], [0] * len(case["img"]))
    _vn, vp, qp, _wx, _bx, _dwv, img, mode = args
    return R.near_zero_count(vp, qp, img, mode)
