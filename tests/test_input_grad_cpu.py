"""CPU: the input-image gradient (v.requires_grad) -- the oracle's autograd d loss / d v against the reference's
(tests/golden/input_grad*.npz, make_golden_input_grad.py), and the new entry points in the header, the ctypes
prototypes and the built library."""
import os
import re

import numpy as np
import pytest
import torch

from tests.golden_util import GOLDEN, TINY_CASES, TRAIN_CASES, Golden, tiny_cfg

NEW_ENTRY_POINTS = ("vqa_conv0_dgrad_supported", "vqa_conv0_dgrad", "vqa_nhwc_to_nchw")


def reference_dv(name):
    """The reference model's d loss / d v for a TINY_CASES / TRAIN_CASES fixture."""
    for f in ("input_grad.npz", "input_grad_k2_stride2.npz"):
        z = np.load(os.path.join(GOLDEN, f))
        if name in z.files:
            return torch.from_numpy(z[name])
    raise KeyError(name)


@pytest.mark.parametrize("name", TINY_CASES + TRAIN_CASES)
def test_oracle_input_grad_matches_reference(name):
    from oracle import vqa_oracle as O
    g = Golden(name)
    masks = g.mask if name in TRAIN_CASES else None
    v = g.t["v"].clone().requires_grad_(True)
    logits = O.vqa_forward(g.sd, tiny_cfg(g.meta), v, g.t["q"], g.t["q_len"], masks=masks)
    loss = O.soft_ce_loss(logits, g.t["a_idx"], g.t["a_val"])
    (dv,) = torch.autograd.grad(loss, v)
    ref = reference_dv(name)
    assert dv.shape == ref.shape
    e = float((dv - ref).abs().max()) / float(ref.abs().max())
    print(f"[input-grad] oracle vs reference {name}: {e:.3e}")
    assert e < 2e-5


def test_full224_input_grad_fixture_is_the_first_sample():
    z = np.load(os.path.join(GOLDEN, "input_grad_full224.npz"))
    assert z["dv0"].shape == (3, 224, 224) and z["dv0"].dtype == np.float32
    assert np.isfinite(z["dv0"]).all() and np.abs(z["dv0"]).max() > 0


def test_new_entry_points_in_header_prototypes_and_library():
    from dl_vqa_amd import _lib
    with open(_lib.HEADER_PATH) as f:
        header = f.read()
    assert _lib.header_abi_version() == 9
    for name in NEW_ENTRY_POINTS:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in _lib.PROTOTYPES, name
    lib = _lib.load()
    assert lib.vqa_abi_version() == 9
    for name in NEW_ENTRY_POINTS:
        assert hasattr(lib, name), name
    # the dedicated path's shape rule: the forward's, minus nothing
    assert lib.vqa_conv0_dgrad_supported(3, 224, 224, 64, 1) == 1
    assert lib.vqa_conv0_dgrad_supported(3, 37, 44, 32, 1) == 1
    assert lib.vqa_conv0_dgrad_supported(4, 224, 224, 64, 1) == 0
    assert lib.vqa_conv0_dgrad_supported(3, 224, 224, 48, 1) == 0
    assert lib.vqa_conv0_dgrad_supported(3, 224, 226, 64, 1) == 0
    assert lib.vqa_conv0_dgrad_supported(3, 224, 224, 64, 2) == 0
