"""Generate the input-gradient fixtures under tests/golden/ from the REFERENCE model.

Run in the build container only, as make_golden.py (it imports the reference and make_golden's helpers):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_input_grad.py

What is recorded (data only):
  input_grad.npz, input_grad_k2_stride2.npz
      "<case>": dv = autograd.grad(loss, v) of the reference model for every TINY_CASES and TRAIN_CASES fixture, with
      the fixture's own inputs, parameters, recorded dropout masks (train cases) and the replayed loss of train.py.
      tiny_k2_stride2 (128 x 128 images) has a file of its own: every file stays under 1 MB.
  input_grad_full224.npz
      "dv0": dv of the first sample of full224_seed1 (the dedicated first-block shape: 3 -> 64 channels, 224 x 224).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_golden as MG  # noqa: E402  (imports the reference model: build container only)
from tests.golden_util import TINY_CASES, TRAIN_CASES, Golden, full_cfg, full_inputs, tiny_cfg  # noqa: E402


def case_dv(name):
    g = Golden(name)
    model = MG.VqaNet(tiny_cfg(g.meta), g.meta["V"])
    model.load_state_dict(g.sd)
    train = name in TRAIN_CASES
    if train:
        m = g.mask
        model.image.drop = MG.MaskDrop([m["image"]])
        model.text.drop = MG.MaskDrop([m["text"]])
        model.attention.drop = MG.MaskDrop([m["att_v"], m["att_q"], m["att_x"]])
        model.classifier.drop1 = MG.MaskDrop([m["cls1"]])
        model.classifier.drop2 = MG.MaskDrop([m["cls2"]])
    model.train(train)
    v = g.t["v"].clone().requires_grad_(True)
    y = model(v, g.t["q"], g.t["q_len"])
    loss = MG.replay_loss(y, g.t["a_idx"], g.t["a_val"], g.t["a_len"])
    assert abs(float(loss.detach()) - float(g.t["loss"])) < 1e-6, name
    (dv,) = torch.autograd.grad(loss, v)
    print(name, "max|dv|", float(dv.abs().max()))
    return dv.detach().numpy()


def full_dv():
    g = Golden("full224_seed1")
    meta = g.meta
    torch.manual_seed(meta["seed"])
    model = MG.VqaNet(full_cfg(meta["A"]), meta["V"]).eval()
    v, q, ql, a_idx, a_val, a_len = full_inputs(meta)
    v = v.requires_grad_(True)
    y = model(v, q, ql)
    loss = MG.replay_loss(y, a_idx, a_val, a_len)
    assert abs(float(loss.detach()) - float(g.t["loss"])) < 1e-5
    (dv,) = torch.autograd.grad(loss, v)
    print("full224 max|dv0|", float(dv[0].abs().max()))
    return dv[0].detach().numpy()


if __name__ == "__main__":
    big = "tiny_k2_stride2"
    np.savez_compressed(os.path.join(HERE, "input_grad.npz"), **{n: case_dv(n) for n in TINY_CASES + TRAIN_CASES if n != big})
    np.savez_compressed(os.path.join(HERE, "input_grad_k2_stride2.npz"), **{big: case_dv(big)})
    np.savez_compressed(os.path.join(HERE, "input_grad_full224.npz"), dv0=full_dv())
