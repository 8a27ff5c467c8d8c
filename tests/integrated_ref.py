"""float64 references for the integrated-gradients maps of VqaNet.explain_integrated / explain_integrated_pairs
(include/vqa_hip.h), built on tests/attribution_ref.py:

  alphas64             the step positions the device uses -- float32((2s + 1) / (2S)) -- widened to float64, so that quadrature
                       error never enters a device comparison;
  riemann_autograd     the Riemann sum by autograd: attribution_ref.autograd_reference on alpha * vn, divided by alpha;
  closed_form_step     the header's formulas at one step, restated (r1_s, dscore_s without the factor alpha, r2_s with it),
                       with the ReLU pre-activations of the scores and of lin1 at that step;
  closed_form          their path sum;
  path_scores / path_attr   what the two kernels compute from given operands;
  path_near_zero_count near_zero_count along the path, and for the lin1 pre-activations;
  completeness         sum of a map over positions against logit[b, a_b] - logit_at_zero_features[b, a_b];
  fixture_reference    the Riemann sum of a golden fixture's pairs, computed once per (fixture, columns, steps).

Everything here runs on the CPU; the GPU tests import it and compute each reference once."""
import functools

import torch

from dl_vqa_amd.model import integrated_alphas
from tests import attribution_ref as R


def alphas64(steps):
    return integrated_alphas(steps).double()


def riemann_autograd(sd, do_option, vn, qf, img, answers, grid, alphas):
    """IG [B, P] = mean_s G_s with G_s = (gradient x input on the cache alpha_s * vn) / alpha_s, by autograd."""
    total = 0
    for a in alphas.tolist():
        total = total + R.autograd_reference(sd, do_option, a * vn.double(), qf, img, answers, grid) / a
    return total / len(alphas)


def closed_form_step(sd, do_option, vn, qf, img, answers, alpha):
    """The header's formulas at x = alpha * vn, in float64: a dict with G, r1, r2 [B, P], dscore, probs [B, G, P], pre (the
    score pre-activation [B, P, mid]) and z (the lin1 pre-activation [B, hid])."""
    sd = R._sd64(sd)
    vn, qf = vn.double(), qf.double()
    mode = R.MODES[do_option]
    wv = sd["attention.v_conv.weight"][:, :, 0, 0]
    wx, bx = sd["attention.x_conv.weight"][:, :, 0, 0], sd["attention.x_conv.bias"]
    G, mid = wx.shape[0], wv.shape[0]
    C = vn.shape[-1]
    vp = vn @ wv.t()
    qp = qf @ sd["attention.q_lin.weight"].t() + sd["attention.q_lin.bias"]
    score, pre = R.scores(alpha * vp, qp, wx, bx, img, mode)
    probs = torch.softmax(score, dim=-1)
    weighted = alpha * torch.einsum("bgp,bpc->bgc", probs, vn[img]).reshape(len(img), G * C)
    w1, w2 = sd["classifier.lin1.weight"], sd["classifier.lin2.weight"]
    z = torch.cat([weighted, qf], dim=1) @ w1.t() + sd["classifier.lin1.bias"]
    dh = w2[torch.as_tensor(answers, dtype=torch.int64)] * (z > 0).double()
    dwv = (dh @ w1[:, :G * C]).view(len(img), G, C)
    out = R.closed_form_from_probs(vn, probs, dwv, img)              # t_s = vn . dwv_s: without the factor alpha
    c = torch.einsum("bgp,gm->bpm", out["dscore"], wx[:, :mid])
    ind = (pre > 0).double()
    s = ind * qp[:, None, :] if mode == 1 else ind
    out["r2"] = alpha * (c * s * vp[img]).sum(-1)
    out["G"] = out["r1"] + out["r2"]
    out.update(probs=probs, pre=pre, z=z)
    return out


def closed_form(sd, do_option, vn, qf, img, answers, alphas):
    """IG [B, P] = (1 / S) * sum_s (r1_s + r2_s)."""
    return sum(closed_form_step(sd, do_option, vn, qf, img, answers, a)["G"] for a in alphas.tolist()) / len(alphas)


def path_scores(vp, qp, wx, bx, img, mode, alphas):
    """[B, S, G, P]: attribution_ref.scores at every alpha_s * v' (what the path-score kernel computes).  vp [N, P, mid]."""
    vp, qp, wx, bx = (x.double() for x in (vp, qp, wx, bx))
    return torch.stack([R.scores(a * vp, qp, wx, bx, img, mode)[0] for a in alphas.double().tolist()], dim=1)


def path_attr(r1, dscore, vp, qp, wx, img, mode, alphas, scale):
    """[B, P]: scale * sum_s score_half(r1[:, s], dscore[:, s]) at alpha_s * v' (what the path-attribution kernel computes)."""
    qp = qp if qp is not None else torch.zeros(r1.shape[0], vp.shape[-1])
    return scale * sum(R.score_half(r1[:, s], dscore[:, s], a * vp.double(), qp, wx, img, mode)
                       for s, a in enumerate(alphas.double().tolist()))


def path_near_zero_count(sd, do_option, vn, qf, img, answers, alphas, rel=R.NEAR_ZERO):
    """(score pre-activations, lin1 pre-activations) of the asked pairs that lie within rel * max|.| of zero at some step,
    the maximum taken per step: where an fp32 evaluation may take the other side of an indicator."""
    n_pre = n_z = 0
    for a in alphas.tolist():
        st = closed_form_step(sd, do_option, vn, qf, img, answers, a)
        n_pre += int((st["pre"].abs() < rel * st["pre"].abs().max()).sum())
        n_z += int((st["z"].abs() < rel * st["z"].abs().max()).sum())
    return n_pre, n_z


def completeness(sd, do_option, vn, qf, img, answers, grid, maps):
    """maps.sum over positions - (logit[b, a_b] - logit_at_zero_features[b, a_b]) in float64, [B]."""
    cols = torch.as_tensor(answers, dtype=torch.int64)[:, None]
    full = R.forward64(sd, do_option, vn, qf, img, grid).gather(1, cols)[:, 0]
    zero = R.forward64(sd, do_option, 0 * vn, qf, img, grid).gather(1, cols)[:, 0]
    return maps.double().reshape(len(img), -1).sum(1) - (full - zero)


def fixture_answers(do_option):
    """The arg-max columns of the fixture's pairs, from the float64 logits."""
    f = R.fixture_case(do_option)
    return R.forward64(f["golden"].sd, do_option, f["vn"], f["qf"], f["img"], f["grid"]).argmax(1).tolist()


@functools.lru_cache(maxsize=None)
def _fixture_reference(do_option, answers, steps):
    f = R.fixture_case(do_option)
    return riemann_autograd(f["golden"].sd, do_option, f["vn"], f["qf"], f["img"], list(answers), f["grid"], alphas64(steps))


def fixture_reference(do_option, answers, steps):
    """The Riemann sum [B, P] of the fixture's pairs for the given answer columns at the device's step positions, computed once
    per (fixture, columns, steps) and shared by the tests that need it."""
    return _fixture_reference(do_option, tuple(int(a) for a in answers), int(steps))


def fixture_gap(do_option, answers, maps):
    """completeness of `maps` [B, P] on the fixture's pairs."""
    f = R.fixture_case(do_option)
    return completeness(f["golden"].sd, do_option, f["vn"], f["qf"], f["img"], list(answers), f["grid"], maps)
