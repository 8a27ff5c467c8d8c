"""The per-batch half of the reference training procedure on the device (train.py:172-208,
utils/train_utils.py:12-25, train.py:31-35,55,80).

``run_batch(model, log_softmax, batch_data, max_answers)``, ``batch_accuracy`` and
``update_learning_rate`` keep the reference's names and argument meaning, so the reference's own
epoch loop (train.py:38-169: ``train`` / ``evaluate``, out of scope here and not restated) calls
them unchanged.  What differs is where the work runs: the soft-target cross entropy, its gradient
and the VQA score are one HIP kernel on the device (the reference builds numpy index arrays on
the host and syncs B+1 times per step, train.py:195-199, train_utils.py:19-23), and ``FusedAdam``
is torch.optim.Adam's update as one kernel over the flat parameter buffer (train.py:55,80).
"""
from __future__ import annotations

from typing import Optional

import torch

from . import ops
from ._lib import ADAM_MAX_SEGMENTS as MAX_ADAM_SEGMENTS     # what one launch carries in its arguments
from .model import _check_index_count, validate_question_lengths


# ------------------------------------------------------------------ loss head
class _SoftCEFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, a_indices, a_values, inv_batch):
        B, A = logits.shape
        dl = torch.empty(B, (A + 3) // 4 * 4, dtype=torch.float32, device=logits.device)
        need_grad = ctx.needs_input_grad[0]
        loss_rows, score_rows = ops.softce(logits, logits.stride(0), a_indices, a_values, A, inv_batch,
                                           dl if need_grad else None, dl.stride(0))
        out = torch.empty(2, dtype=torch.float32, device=logits.device)
        ops.colsum(loss_rows, B, 1, out[0:1])
        ops.colsum(score_rows, B, 1, out[1:2])
        ctx.dl = dl if need_grad else None
        ctx.A = A
        loss, score = out[0], out[1]
        ctx.mark_non_differentiable(score)
        return loss, score

    @staticmethod
    def backward(ctx, g_loss, g_score):
        dl = ctx.dl
        ops.scale_by(dl, g_loss.contiguous())
        return dl[:, :ctx.A], None, None, None


def soft_ce_loss_and_score(logits: torch.Tensor, a_indices: torch.Tensor, a_values: torch.Tensor,
                           batch_divisor: Optional[int] = None):
    """(loss, score): train.py:190-206 and train_utils.py:12-25 on the device.

    loss = sum_{b,k} -log_softmax(logits)[b, a_idx[b,k]-1] * a_val[b,k]/10 / batch_divisor
    score = sum_b min(1, 0.3 * count of the arg-max answer)."""
    dev = logits.device
    a_indices = a_indices.to(device=dev, dtype=torch.int64).contiguous()
    a_values = a_values.to(device=dev, dtype=torch.int64).contiguous()
    div = float(batch_divisor if batch_divisor is not None else logits.shape[0])
    return _SoftCEFunction.apply(logits, a_indices, a_values, 1.0 / div)


def batch_accuracy(predicted, true):
    """utils/train_utils.py:12-25 signature: true = (indices, values, size)."""
    indices, values, _size = true
    dev = predicted.device
    _, score = soft_ce_loss_and_score(predicted.detach(), indices.to(dev), values.to(dev))
    return score


def run_batch(model, log_softmax, batch_data, max_answers, batch_divisor: Optional[int] = None):
    """Reference signature (train.py:172-208). `log_softmax` is accepted and unused: the fused loss
    kernel computes log-softmax, the sparse soft-target cross entropy and the score in one pass.

    The loss is divided by the batch (train.py:206).  Under data parallelism (the model carries a
    dl_vqa_amd.distributed.DataParallel synchroniser) the divisor defaults to the GLOBAL batch, local batch x
    world size, because the gradients are SUM-all-reduced: the reference's own loop, which calls
    run_batch(model, log_softmax, batch_data, max_answers) with no divisor (train.py:70-73), then trains on the
    mean over the global batch exactly as it does on one GPU."""
    v, q, a_indices, a_values, a_length, idx, q_len = batch_data
    dev = next(model.parameters()).device
    if batch_divisor is None:
        sync = getattr(model, "_grad_sync", None)
        if sync is not None:
            batch_divisor = int(v.shape[0]) * int(sync.world_size)
    v = v.to(dev, non_blocking=True)
    q = q.to(dev, non_blocking=True)
    a_indices = a_indices.to(dev, non_blocking=True)
    a_values = a_values.to(dev, non_blocking=True)
    validate_question_lengths(q_len, q.shape[1])       # host-resident lengths: the error pack_padded_sequence would raise
    q_len = q_len.to(dev, non_blocking=True)
    # the dataset stores fp16 features (data_preprocessing.py:174 casts them on the host, per sample): the fp16
    # batch goes over PCIe as is and the first-block kernels read it as it is (widened where their LDS patch is staged)
    if v.dtype not in (torch.float32, torch.float16):
        v = v.float()
    y_hat = model(v, q, q_len)
    batch_loss, batch_score = soft_ce_loss_and_score(y_hat, a_indices, a_values, batch_divisor)
    return batch_loss, batch_score


def run_batch_shared(model, batch_data, max_answers, image_index, batch_divisor: Optional[int] = None):
    """run_batch for a batch whose images are deduplicated: batch_data is the loader's 7-tuple with v [N,3,S,S] holding
    every image once, everything else per question; question b looks at image image_index[b] (a host list or an integer
    tensor of B entries in [0, N)).  Same fused loss and score; the loss is divided by the number of QUESTIONS
    (train.py:206 divides by the batch, and a sample of the reference's batch is a question).  The conv blocks and v_conv
    run once per image, forward and backward (VqaNet.forward_shared, which also states the dropout semantics)."""
    v, q, a_indices, a_values, a_length, idx, q_len = batch_data
    n_index = len(image_index) if not torch.is_tensor(image_index) else image_index.numel()
    _check_index_count("run_batch_shared", n_index, q.shape[0])
    dev = next(model.parameters()).device
    v = v.to(dev, non_blocking=True)
    q = q.to(dev, non_blocking=True)
    a_indices = a_indices.to(dev, non_blocking=True)
    a_values = a_values.to(dev, non_blocking=True)
    validate_question_lengths(q_len, q.shape[1])
    q_len = q_len.to(dev, non_blocking=True)
    if v.dtype not in (torch.float32, torch.float16):
        v = v.float()
    y_hat = model.forward_shared(v, q, q_len, image_index)
    return soft_ce_loss_and_score(y_hat, a_indices, a_values, batch_divisor)


def run_batch_features(model, batch_data, max_answers, feats, image_index, batch_divisor: Optional[int] = None,
                       image_dropout=False):
    """run_batch_shared with the image encoder frozen and run beforehand: `feats` (VqaNet.encode_images, a bank of N feature
    rows) stands in for the images and question b looks at row image_index[b] (a host list or an integer tensor of B
    entries in [0, N)).  batch_data is the loader's 7-tuple; its v entry is ignored and may be None.  Same fused loss and
    score; the loss is divided by the number of QUESTIONS.  No convolution runs, and the image.* parameters get no gradient
    (VqaNet.forward_features, which also states the dropout semantics).  The bank may be stored as float16
    (encode_images(..., dtype=torch.float16): half the memory); the step is then, bit for bit, the step on the fp32 bank
    holding the same values.

    image_dropout=True (a bool; ValueError otherwise) applies image.drop at the configured rate to the asked rows, which are
    renormalised after it: the head then trains on what run_batch_shared gives it with image.* frozen, instead of on
    features that image.drop never touched (VqaNet.forward_features).  The default leaves the step as it was."""
    if not isinstance(image_dropout, bool):
        raise ValueError(f"run_batch_features: image_dropout must be a bool, got {image_dropout!r}")
    _v, q, a_indices, a_values, a_length, idx, q_len = batch_data
    n_index = len(image_index) if not torch.is_tensor(image_index) else image_index.numel()
    _check_index_count("run_batch_features", n_index, q.shape[0])
    dev = next(model.parameters()).device
    q = q.to(dev, non_blocking=True)
    a_indices = a_indices.to(dev, non_blocking=True)
    a_values = a_values.to(dev, non_blocking=True)
    validate_question_lengths(q_len, q.shape[1])
    q_len = q_len.to(dev, non_blocking=True)
    y_hat = model.forward_features(feats, q, q_len, image_index, image_dropout)
    return soft_ce_loss_and_score(y_hat, a_indices, a_values, batch_divisor)


# ------------------------------------------------------------------ optimiser
def update_learning_rate(optimizer, iteration, initial_lr):
    """train.py:31-35."""
    lr_halflife = 50000
    lr = initial_lr * 0.5 ** (float(iteration) / lr_halflife)
    for param_group in optimizer.param_groups:
        param_group["lr"] = lr


_GROUP_KEYS = ("params", "lr_scale", "weight_decay", "decoupled", "frozen", "betas", "eps")


def _matches(name: str, spec: str) -> bool:
    """A group's `params` entry names a parameter ("text.embedding.weight") or a prefix of dotted names ("image", "text.embedding")."""
    return name == spec or name.startswith(spec + ".")


class FusedAdam:
    """torch.optim.Adam(model.parameters(), lr) defaults (betas 0.9/0.999, eps 1e-8, no weight decay)
    as ONE kernel over the model's flat parameter / gradient buffers.

    ``groups=None`` (the default) is that optimiser: one group, one global step count, ``ops.adam`` over the whole buffer.

    ``groups=[{...}, ...]`` gives torch.optim.Adam's parameter groups, still as one launch per step (``ops.adam_segments``
    walks a table of ranges of the flat buffer).  Each dict has ``params`` -- a parameter name, a prefix of dotted names
    such as ``"image"`` or ``"text.embedding"``, or a list of those, matched against ``model.named_parameters()`` -- and
    optionally ``lr_scale`` (1.0), ``weight_decay`` (0.0), ``decoupled`` (False: L2 decay as torch.optim.Adam; True:
    torch.optim.AdamW), ``frozen`` (False), ``betas`` and ``eps`` (the constructor's).  A parameter matched by two groups and
    an entry that matches nothing raise ValueError; parameters matched by no group form a last group with the constructor's
    values.  There is no amsgrad.

    ``param_groups[k]["lr"]`` is the schedule's rate, the same in every group, because the reference's
    ``update_learning_rate`` writes one value into all of them (train.py:31-35); what differs per group lives in
    ``lr_scale`` and the rate a group's parameters are updated with is ``lr * lr_scale``.

    Every parameter has its own step number, as in torch: it advances in exactly the steps that update the parameter -- it
    has a gradient and its group is not frozen -- so a parameter that joins late (``unfreeze``) starts its bias correction
    at step 1.  Parameters that are not updated are not listed in the table: the kernel neither reads nor writes them.
    ``state_dict()`` is torch.optim.Adam's, with a state entry only for parameters that have been updated."""

    def __init__(self, model, lr: float, betas=(0.9, 0.999), eps: float = 1e-8, *, groups=None):
        self.model = model
        self.step_count = 0
        self.exp_avg = None
        self.exp_avg_sq = None
        self.grouped = groups is not None
        if not self.grouped:
            self.param_groups = [{"lr": lr, "betas": betas, "eps": eps}]
            return
        names = [n for n, _ in model.named_parameters()]
        owner = {}
        self.param_groups = []
        for k, spec in enumerate(groups):
            unknown = set(spec) - set(_GROUP_KEYS)
            if unknown or "params" not in spec:
                raise ValueError(f"FusedAdam: group {k} needs 'params' and may set {_GROUP_KEYS[1:]}; got {sorted(spec)}")
            entries = (spec["params"],) if isinstance(spec["params"], str) else tuple(spec["params"])
            members = []
            for e in entries:
                hit = [n for n in names if _matches(n, e)]
                if not hit:
                    raise ValueError(f"FusedAdam: group {k}: {e!r} matches no parameter")
                for n in hit:
                    if n in owner:
                        raise ValueError(f"FusedAdam: parameter {n} is matched by group {owner[n]} and by group {k}")
                    owner[n] = k
                members += hit
            self.param_groups.append({
                "lr": lr, "betas": tuple(spec.get("betas", betas)), "eps": spec.get("eps", eps),
                "weight_decay": float(spec.get("weight_decay", 0.0)), "lr_scale": float(spec.get("lr_scale", 1.0)),
                "frozen": bool(spec.get("frozen", False)), "decoupled": bool(spec.get("decoupled", False)),
                "spec": entries, "params": [n for n in names if n in members]})
        rest = [n for n in names if n not in owner]
        if rest:
            self.param_groups.append({"lr": lr, "betas": tuple(betas), "eps": eps, "weight_decay": 0.0, "lr_scale": 1.0,
                                      "frozen": False, "decoupled": False, "spec": (), "params": rest})
        self.steps = {n: 0 for n in names}       # per parameter: the number of updates it has had

    def _require_groups(self, what):
        if not self.grouped:
            raise RuntimeError(f"FusedAdam.{what} needs parameter groups: build the optimiser with groups=[...]")

    def _set_frozen(self, prefix, value):
        self._require_groups("freeze / unfreeze")
        spec = (prefix,) if isinstance(prefix, str) else tuple(prefix)
        hit = [g for g in self.param_groups if g["spec"] == spec]
        if not hit:
            raise ValueError(f"FusedAdam: no group was built with params={prefix!r} "
                             f"(groups: {[list(g['spec']) for g in self.param_groups if g['spec']]})")
        hit[0]["frozen"] = value

    def freeze(self, prefix):
        """Stop updating the group that was built with params=prefix (the same as param_groups[k]["frozen"] = True): its
        values, moments and step numbers stay as they are, whether or not its parameters get gradients."""
        self._set_frozen(prefix, True)

    def unfreeze(self, prefix):
        """Update that group again; its parameters go on from their own step numbers (from 1 if they never were updated)."""
        self._set_frozen(prefix, False)

    def _state(self):
        flat_p, flat_g, _ = self.model.flat_buffers()
        if self.exp_avg is None or self.exp_avg.numel() != flat_p.numel() or self.exp_avg.device != flat_p.device:
            self.exp_avg = torch.zeros_like(flat_p)
            self.exp_avg_sq = torch.zeros_like(flat_p)
        return flat_p, flat_g

    def zero_grad(self, set_to_none: bool = True):
        """torch.optim.Optimizer.zero_grad semantics.  set_to_none=True (torch's default) drops the gradients:
        the next backward then writes straight into the flat buffer (the fast path, and the one whose bucket
        all-reduces see the model's own buffer).  set_to_none=False zeroes existing gradients in place, as torch
        does; the next backward then goes through a fresh buffer that autograd ADDS to them (correct, one extra
        buffer pass per step)."""
        for p in self.model.parameters():
            if set_to_none or p.grad is None:
                p.grad = None
            else:
                p.grad.detach_()
                p.grad.requires_grad_(False)
                p.grad.zero_()

    def _gather_grads(self, flat_g):
        """The kernel reads the model's flat gradient buffer.  After a plain backward every p.grad IS a view
        of it; after gradient accumulation (or anything else that made autograd allocate its own p.grad) the
        gradients are copied into their slots first.  Returns the names of parameters WITHOUT a gradient (frozen
        with requires_grad=False, or unused): torch.optim.Adam skips those (train.py:55,80), so step() leaves their
        values and moments untouched."""
        _, _, offsets = self.model.flat_buffers()
        named = list(self.model.named_parameters())
        missing = [n for n, p in named if p.grad is None]
        if len(missing) == len(named):
            raise RuntimeError("FusedAdam.step: no parameter has a gradient: run backward first")
        base = flat_g.data_ptr()
        for n, p in named:
            o, k = offsets[n]
            if p.grad is None:
                flat_g[o:o + k].zero_()
            elif p.grad.data_ptr() != base + 4 * o or not p.grad.is_contiguous():
                flat_g[o:o + k].view(p.shape).copy_(p.grad)
        return missing

    def _segments(self, flat_g):
        """The table of one grouped step: a segment per parameter that is updated -- it has a gradient and its group is not
        frozen -- over its padded slot [offset, offset + ceil64(numel)) (the pad is zero in every buffer and stays zero under
        Adam with or without decay), sorted by offset, neighbours with equal settings and step merged.  Gradients that
        autograd keeps outside the flat buffer are copied into their slots (_gather_grads's rule); the slots of parameters
        that are not updated are left alone.  Returns (segments, names of the updated parameters)."""
        _, _, offsets = self.model.flat_buffers()
        named = dict(self.model.named_parameters())
        if all(p.grad is None for p in named.values()):
            raise RuntimeError("FusedAdam.step: no parameter has a gradient: run backward first")
        base = flat_g.data_ptr()
        slots, updated = [], []
        for g in self.param_groups:
            if g["frozen"]:
                continue
            for n in g["params"]:
                p = named[n]
                if p.grad is None:
                    continue
                o, k = offsets[n]
                if p.grad.data_ptr() != base + 4 * o or not p.grad.is_contiguous():
                    flat_g[o:o + k].view(p.shape).copy_(p.grad)
                settings = (g["lr"] * g["lr_scale"], g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"],
                            self.steps[n] + 1, int(g["decoupled"]))
                slots.append((o, o + (k + 63) // 64 * 64, settings))
                updated.append(n)
        if not slots:
            raise RuntimeError("FusedAdam.step: no parameter has a gradient: every parameter with one is in a frozen group")
        slots.sort(key=lambda s: s[0])
        segments = []
        for begin, end, settings in slots:
            if segments and segments[-1][1] == begin and segments[-1][2:] == settings:
                segments[-1] = (segments[-1][0], end) + settings
            else:
                segments.append((begin, end) + settings)
        if len(segments) > MAX_ADAM_SEGMENTS:
            raise RuntimeError(f"FusedAdam.step: {len(segments)} segments with different settings or steps; one launch "
                               f"carries {MAX_ADAM_SEGMENTS}")
        return segments, updated

    def step(self, grad_scale: float = 1.0):
        if self.grouped:
            flat_p, flat_g = self._state()
            segments, updated = self._segments(flat_g)
            ops.adam_segments(flat_p, flat_g, self.exp_avg, self.exp_avg_sq, segments, grad_scale)
            for n in updated:
                self.steps[n] += 1
            return
        flat_p, flat_g = self._state()
        missing = self._gather_grads(flat_g)
        g = self.param_groups[0]
        self.step_count += 1
        keep = []
        if missing:      # skipped parameters keep value AND moments (the kernel updates the whole buffer)
            _, _, offsets = self.model.flat_buffers()
            for n in missing:
                o, k = offsets[n]
                keep.append((o, k, flat_p[o:o + k].clone(), self.exp_avg[o:o + k].clone(), self.exp_avg_sq[o:o + k].clone()))
        ops.adam(flat_p, flat_g, self.exp_avg, self.exp_avg_sq, g["lr"], self.step_count, g["betas"][0],
                 g["betas"][1], g["eps"], grad_scale)
        for o, k, pv, m1, m2 in keep:
            flat_p[o:o + k].copy_(pv)
            self.exp_avg[o:o + k].copy_(m1)
            self.exp_avg_sq[o:o + k].copy_(m2)

    # checkpoint format of torch.optim.Adam, so `optimizer_state` in model.pth interchanges
    # (utils/train_logger.py:95-112, train.py:56-57)
    def _grouped_state_dict(self):
        """torch.optim.Adam's format: a param_groups entry per group with `params` as indices into named_parameters(), and
        state[i] only for parameters that have been updated (step >= 1), each with its own step.  `lr` is the schedule's
        rate; lr_scale, frozen and decoupled ride along (torch keeps keys it does not know).  torch.optim.Adam built with the
        same grouping loads the result (AdamW for groups with decoupled=True); it knows no lr_scale, so whoever hands the
        dict to torch multiplies each group's lr by its lr_scale."""
        self._state()
        _, _, offsets = self.model.flat_buffers()
        named = list(self.model.named_parameters())
        index = {n: i for i, (n, _) in enumerate(named)}
        state = {}
        for i, (n, p) in enumerate(named):
            if self.steps[n] >= 1:
                o, k = offsets[n]
                state[i] = {"step": torch.tensor(float(self.steps[n])),
                            "exp_avg": self.exp_avg[o:o + k].view(p.shape).clone(),
                            "exp_avg_sq": self.exp_avg_sq[o:o + k].view(p.shape).clone()}
        groups = [{"lr": g["lr"], "betas": g["betas"], "eps": g["eps"], "weight_decay": g["weight_decay"], "amsgrad": False,
                   "lr_scale": g["lr_scale"], "frozen": g["frozen"], "decoupled": g["decoupled"],
                   "params": [index[n] for n in g["params"]]} for g in self.param_groups]
        return {"state": state, "param_groups": groups}

    def _load_grouped_state_dict(self, sd):
        self._state()
        _, _, offsets = self.model.flat_buffers()
        names = [n for n, _ in self.model.named_parameters()]
        index = {n: i for i, n in enumerate(names)}
        if len(sd["param_groups"]) != len(self.param_groups):
            raise ValueError(f"FusedAdam.load_state_dict: {len(sd['param_groups'])} groups for an optimiser with "
                             f"{len(self.param_groups)}")
        for k, (g, saved) in enumerate(zip(self.param_groups, sd["param_groups"])):
            if list(saved["params"]) != [index[n] for n in g["params"]]:
                raise ValueError(f"FusedAdam.load_state_dict: group {k} holds other parameters than the optimiser's group {k}")
        for g, saved in zip(self.param_groups, sd["param_groups"]):
            g.update(lr=saved["lr"], betas=tuple(saved["betas"]), eps=saved["eps"],
                     weight_decay=float(saved.get("weight_decay", 0.0)), lr_scale=float(saved.get("lr_scale", 1.0)),
                     frozen=bool(saved.get("frozen", False)), decoupled=bool(saved.get("decoupled", False)))
        for i, n in enumerate(names):
            o, k = offsets[n]
            st = sd["state"].get(i)
            if st is None:                      # never updated: no moments, step 0
                self.exp_avg[o:o + k].zero_()
                self.exp_avg_sq[o:o + k].zero_()
                self.steps[n] = 0
            else:
                self.exp_avg[o:o + k].copy_(st["exp_avg"].reshape(-1))
                self.exp_avg_sq[o:o + k].copy_(st["exp_avg_sq"].reshape(-1))
                self.steps[n] = int(float(st["step"]))

    def state_dict(self):
        if self.grouped:
            return self._grouped_state_dict()
        flat_p, _ = self._state()
        _, _, offsets = self.model.flat_buffers()
        state = {}
        names = [n for n, _ in self.model.named_parameters()]
        for i, n in enumerate(names):
            o, k = offsets[n]
            shape = dict(self.model.named_parameters())[n].shape
            state[i] = {"step": torch.tensor(float(self.step_count)),
                        "exp_avg": self.exp_avg[o:o + k].view(shape).clone(),
                        "exp_avg_sq": self.exp_avg_sq[o:o + k].view(shape).clone()}
        g = self.param_groups[0]
        group = {"lr": g["lr"], "betas": g["betas"], "eps": g["eps"], "weight_decay": 0, "amsgrad": False,
                 "params": list(range(len(names)))}
        return {"state": state, "param_groups": [group]}

    def load_state_dict(self, sd):
        if self.grouped:
            return self._load_grouped_state_dict(sd)
        self._state()
        _, _, offsets = self.model.flat_buffers()
        names = [n for n, _ in self.model.named_parameters()]
        for i, n in enumerate(names):
            if i not in sd["state"]:
                continue
            o, k = offsets[n]
            st = sd["state"][i]
            self.exp_avg[o:o + k].copy_(st["exp_avg"].reshape(-1))
            self.exp_avg_sq[o:o + k].copy_(st["exp_avg_sq"].reshape(-1))
            self.step_count = int(float(st["step"]))
        g = sd["param_groups"][0]
        self.param_groups[0].update(lr=g["lr"], betas=tuple(g["betas"]), eps=g["eps"])
