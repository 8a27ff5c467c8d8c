"""References for FusedAdam's parameter groups and the segmented Adam kernel.  Nothing here touches the GPU or the HIP library.

adam_segments_f64 is ops.adam_segments restated in float64 on CPU tensors (the scalars at the float32 values the C ABI
passes, as tests/streaming_ref.py::adam_ref takes them); TorchTwin is torch.optim.Adam on float64 copies of a model's
parameters, built with the same grouping and fed the gradients the model has.
"""
import numpy as np
import torch

from dl_vqa_amd import ops
from tests import streaming_ref as R

ADAM_TOL = 1e-6          # the project's Adam bound: tests/test_streaming_gpu.py, check("adam ...", p, ref, 1e-6)


def f32(x) -> float:
    return float(np.float32(x))


def check(name, got, ref, tol=ADAM_TOL):
    """tests/test_streaming_gpu.py::check: max|got - ref| / max|ref| within tol, and nothing non-finite."""
    e = R.rel_err(got, ref)
    print(f"[parity] {name}: max|err|/max|ref| = {e:.3e} (tol {tol:.1e})")
    assert bool(torch.isfinite(got).all()), f"{name}: non-finite elements"
    assert e <= tol, f"{name}: {e} > {tol}"
    return e


def as_dicts(segments):
    return [s if isinstance(s, dict) else dict(zip(ops.ADAM_SEGMENT_FIELDS, s)) for s in segments]


def adam_segments_f64(param, grad, exp_avg, exp_avg_sq, segments, grad_scale=1.0):
    """The table in float64, in place on float32 (or float64) CPU buffers: torch.optim.Adam's update per segment with the
    gradient scale, L2 decay (grad + wd * param) or decoupled decay (param * (1 - lr * wd) first)."""
    for s in as_dicts(segments):
        sl = slice(int(s["begin"]), int(s["end"]))
        lr, b1, b2, eps = f32(s["lr"]), f32(s.get("beta1", 0.9)), f32(s.get("beta2", 0.999)), f32(s.get("eps", 1e-8))
        wd, step = f32(s.get("weight_decay", 0.0)), int(s.get("step", 1))
        p, g = param[sl].double(), grad[sl].double() * f32(grad_scale)
        m, v = exp_avg[sl].double(), exp_avg_sq[sl].double()
        if wd != 0.0:
            if s.get("decoupled", 0):
                p = p * (1.0 - lr * wd)
            else:
                g = g + wd * p
        m = b1 * m + (1.0 - b1) * g
        v = b2 * v + (1.0 - b2) * g * g
        denom = v.sqrt() / np.sqrt(1.0 - b2 ** step) + eps
        p = p - (lr / (1.0 - b1 ** step)) * (m / denom)
        param[sl], exp_avg[sl], exp_avg_sq[sl] = p.to(param.dtype), m.to(exp_avg.dtype), v.to(exp_avg_sq.dtype)


class TorchTwin:
    """torch.optim.Adam (AdamW where every group is decoupled) over float64 copies of a model's parameters, one torch group
    per FusedAdam group with lr = lr * lr_scale.  step(opt) hands every parameter the model's current gradient, except
    those of groups that `opt` has frozen (torch then skips them, as it skips every parameter without a gradient)."""

    def __init__(self, model, opt):
        self.names = [n for n, _ in model.named_parameters()]
        self.params = {n: p.detach().double().cpu().clone().requires_grad_(True) for n, p in model.named_parameters()}
        groups = [{"params": [self.params[n] for n in g["params"]], "lr": g["lr"] * g["lr_scale"], "betas": g["betas"],
                   "eps": g["eps"], "weight_decay": g["weight_decay"]} for g in opt.param_groups]
        decoupled = [g["decoupled"] and g["weight_decay"] != 0.0 for g in opt.param_groups]
        assert all(decoupled) or not any(decoupled), "one torch optimiser: Adam or AdamW"
        self.opt = (torch.optim.AdamW if any(decoupled) else torch.optim.Adam)(groups, lr=opt.param_groups[0]["lr"])

    def step(self, model, opt, grad_scale=1.0):
        frozen = {n for g in opt.param_groups if g["frozen"] for n in g["params"]}
        for n, p in model.named_parameters():
            t = self.params[n]
            t.grad = None if p.grad is None or n in frozen else p.grad.detach().double().cpu() * f32(grad_scale)
        for tg, g in zip(self.opt.param_groups, opt.param_groups):
            tg["lr"] = g["lr"] * g["lr_scale"]
        self.opt.step()

    def steps(self):
        """{index in named_parameters(): step} of the parameters torch holds state for."""
        out = {}
        for i, n in enumerate(self.names):
            st = self.opt.state.get(self.params[n])
            if st:
                out[i] = int(float(st["step"]))
        return out
