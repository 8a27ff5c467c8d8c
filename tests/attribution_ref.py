"""float64 references for the gradient x input maps of VqaNet.explain / explain_pairs (include/vqa_hip.h):

  closed_form          the header's formulas restated from (vn, v', q', wx, bx, dwv, img, mode);
  autograd_reference   (vn * d logit[b, a_b] / d vn).sum(channels) by torch.autograd through the oracle's differentiable
                       pieces (attention_scores, image_question_attention, classifier), vn[img] as the leaf;
  model_inputs         what closed_form needs, from a state dict: v', q' and dwv through the eval-mode classifier;
  near_zero_count      how many ReLU pre-activations lie within rounding of zero (the indicators s are discontinuous there);
  fixture_case         the (image, question) pairs the GPU tests ask of a golden fixture, with their float64 features.

Everything here runs on the CPU; the GPU tests import it and compute each reference once."""
import functools

import torch

from oracle import vqa_oracle as O
from tests.golden_util import Golden, tiny_cfg

MODES = {"+": 0, "*": 1, "|": 2}
# one golden fixture per do_option, and the pairs asked of its first three images: repeats, any order, more questions than
# images, every image asked (tests/test_multi_question_gpu.py item 7 asks the same)
FIXTURES = {"+": "tiny_plus", "*": "tiny_mul", "|": "tiny_cat"}
IMAGE_INDEX = (0, 1, 2, 2, 0, 1, 1)
QUESTION_SEL = (0, 1, 2, 0, 1, 2, 1)
NEAR_ZERO = 1e-5


def scores(vp, qp, wx, bx, img, mode):
    """[B, G, P] and the pre-activation [B, P, mid] ('|': of the v' half) from v' [N, P, mid], q' [B, mid]."""
    mid = vp.shape[-1]
    v, q = vp[img], qp[:, None, :]
    if mode == 0:
        pre = v + q
        s = torch.relu(pre) @ wx.t()
    elif mode == 1:
        pre = v * q
        s = torch.relu(pre) @ wx.t()
    else:
        pre = v
        s = torch.relu(v) @ wx[:, :mid].t() + torch.relu(q) @ wx[:, mid:].t()
    return (s + bx).permute(0, 2, 1), pre


def closed_form(vn, vp, qp, wx, bx, dwv, img, mode):
    """The header's formulas in float64.  vn [N, P, C], vp [N, P, mid], qp [B, mid], wx [G, xld], bx [G], dwv [B, G, C],
    img int64 [B].  Returns a dict: R, r1, r2 [B, P], dscore, probs [B, G, P], rowsum [B, G]."""
    vn, vp, qp, wx, bx, dwv = (x.double() for x in (vn, vp, qp, wx, bx, dwv))
    mid = vp.shape[-1]
    score, pre = scores(vp, qp, wx, bx, img, mode)
    probs = torch.softmax(score, dim=-1)
    out = closed_form_from_probs(vn, probs, dwv, img)
    c = torch.einsum("bgp,gm->bpm", out["dscore"], wx[:, :mid])
    ind = (pre > 0).double()
    s = ind * qp[:, None, :] if mode == 1 else ind
    out["r2"] = (c * s * vp[img]).sum(-1)
    out["R"] = out["r1"] + out["r2"]
    out["probs"] = probs
    return out


def closed_form_from_probs(vn, probs, dwv, img):
    """The weighted-sum half: t, r1, dscore and its row sums from given probabilities (what kernel 1 computes)."""
    vn, probs, dwv = vn.double(), probs.double(), dwv.double()
    t = torch.einsum("bpc,bgc->bgp", vn[img], dwv)
    dscore = probs * (t - (probs * t).sum(-1, keepdim=True))
    return {"t": t, "r1": (probs * t).sum(1), "dscore": dscore, "rowsum": dscore.sum(-1)}


def score_half(r1, dscore, vp, qp, wx, img, mode):
    """R = r1 + r2 from given r1 and dscore (what kernel 2 computes).  vp [N, P, mid]."""
    r1, dscore, vp, qp, wx = (x.double() for x in (r1, dscore, vp, qp, wx))
    mid = vp.shape[-1]
    v, q = vp[img], qp[:, None, :]
    c = torch.einsum("bgp,gm->bpm", dscore, wx[:, :mid])
    s = (v + q > 0).double() if mode == 0 else ((v * q > 0).double() * q if mode == 1 else (v > 0).double())
    return r1 + (c * s * v).sum(-1)


def _sd64(sd):
    return {k: (t.double() if t.is_floating_point() else t) for k, t in sd.items()}


def _as_maps(vb, grid):
    """[B, P, C] -> the oracle's [B, C, gh, gw]."""
    B, P, C = vb.shape
    return vb.permute(0, 2, 1).reshape(B, C, *grid)


def forward64(sd, do_option, vn, qf, img, grid):
    """Eval-mode logits [B, A] in float64 from vn [N, P, C] and the question features qf [B, Q]."""
    sd = _sd64(sd)
    v = _as_maps(vn.double()[img], grid)
    att = O.attention_scores(sd, v, qf.double(), do_option)
    wv, _ = O.image_question_attention(v, att)
    return O.classifier(sd, torch.cat([wv, qf.double()], dim=1))


def autograd_reference(sd, do_option, vn, qf, img, answers, grid):
    """R [B, P] by autograd: the leaf is vn[img] (one copy of the features per question, so that questions about the same
    image do not share a gradient); the question features are constants."""
    sd = _sd64(sd)
    vb = vn.double()[img].clone().requires_grad_(True)
    v = _as_maps(vb, grid)
    att = O.attention_scores(sd, v, qf.double(), do_option)
    wv, _ = O.image_question_attention(v, att)
    logits = O.classifier(sd, torch.cat([wv, qf.double()], dim=1))
    picked = logits.gather(1, torch.as_tensor(answers, dtype=torch.int64)[:, None]).sum()
    (grad,) = torch.autograd.grad(picked, vb)
    return (vb.detach() * grad).sum(-1)


def model_inputs(sd, do_option, vn, qf, img, answers):
    """closed_form's arguments from a state dict: (vn, v' [N, P, mid], q', wx, bx, dwv [B, G, C], img, mode) -- v' and q' by
    their products, dwv = d logit[b, a_b] / d combined[:, :GC] through the eval-mode classifier."""
    sd = _sd64(sd)
    vn, qf = vn.double(), qf.double()
    N, P, C = vn.shape
    mode = MODES[do_option]
    wv = sd["attention.v_conv.weight"][:, :, 0, 0]
    wx, bx = sd["attention.x_conv.weight"][:, :, 0, 0], sd["attention.x_conv.bias"]
    G = wx.shape[0]
    vp = vn @ wv.t()
    qp = qf @ sd["attention.q_lin.weight"].t() + sd["attention.q_lin.bias"]
    score, _ = scores(vp, qp, wx, bx, img, mode)
    probs = torch.softmax(score, dim=-1)
    weighted = torch.einsum("bgp,bpc->bgc", probs, vn[img]).reshape(len(img), G * C)
    w1, w2 = sd["classifier.lin1.weight"], sd["classifier.lin2.weight"]
    h1 = torch.relu(torch.cat([weighted, qf], dim=1) @ w1.t() + sd["classifier.lin1.bias"])
    dh = w2[torch.as_tensor(answers, dtype=torch.int64)] * (h1 > 0).double()
    dwv = (dh @ w1[:, :G * C]).view(len(img), G, C)
    return vn, vp, qp, wx, bx, dwv, img, mode


def near_zero_count(vp, qp, img, mode, rel=NEAR_ZERO):
    """Elements of the ReLU pre-activation (v' + q', v' * q', or v' for '|') of the asked pairs with magnitude below
    rel * max|.|: where an fp32 evaluation may take the other side of the indicator."""
    v, q = vp.double()[img], qp.double()[:, None, :]
    pre = v + q if mode == 0 else (v * q if mode == 1 else v)
    return int((pre.abs() < rel * pre.abs().max()).sum())


@functools.lru_cache(maxsize=None)
def fixture_case(do_option):
    """The golden fixture of `do_option` with the pairs the GPU tests ask of it: a dict with the Golden, its cfg, the first
    three images' float64 features vn [3, P, C] and grid, the asked questions' tokens, lengths and float64 features, and
    the image index."""
    g = Golden(FIXTURES[do_option])
    cfg = tiny_cfg(g.meta)
    assert cfg["attention"]["do_option"] == do_option
    sd = _sd64(g.sd)
    img = torch.tensor(IMAGE_INDEX)
    qsel = torch.tensor(QUESTION_SEL)
    v, q, ql = g.t["v"][:3], g.t["q"][qsel], g.t["q_len"][qsel]
    x = O.l2_normalise(O.image_encoder(sd, v.double(), cfg["image"]["stride"]))         # [3, C, gh, gw]
    grid = tuple(x.shape[2:])
    vn = x.reshape(x.shape[0], x.shape[1], -1).permute(0, 2, 1).contiguous()
    qf = O.question_encoder(sd, q, ql, cfg["text"]["bidirectional"])
    return {"golden": g, "cfg": cfg, "v": v, "q": q, "q_len": ql, "img": img, "vn": vn, "qf": qf, "grid": grid}


@functools.lru_cache(maxsize=None)
def _fixture_reference(do_option, answers):
    f = fixture_case(do_option)
    sd = f["golden"].sd
    ref = autograd_reference(sd, do_option, f["vn"], f["qf"], f["img"], list(answers), f["grid"])
    parts = closed_form(*model_inputs(sd, do_option, f["vn"], f["qf"], f["img"], list(answers)))
    return ref, parts["r1"], parts["r2"]


def fixture_reference(do_option, answers):
    """(R by autograd, r1, r2 by the closed form) [B, P] of the fixture's pairs for the given answer columns, computed once
    per (fixture, columns) and shared by the tests that need it."""
    return _fixture_reference(do_option, tuple(int(a) for a in answers))
