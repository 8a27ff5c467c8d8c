"""CPU: image dropout when training on cached image features -- the identity the feature rests on (dropping and
renormalising the cached, normalised features is dropping the pooled features and normalising them: tests/feature_dropout_ref.py
against the reference's own order), the host-side argument validation of vqa_gather_rows_drop_norm and its _f16 form with
made-up aligned pointers (every check runs before any HIP call, nothing dereferences them), and the type check of the
image_dropout argument, which comes before any device work."""
import pytest
import torch

from dl_vqa_amd import VqaNet
from tests.feature_dropout_ref import drop_norm, kept_norms, l2norm, oracle_drop_then_norm
from tests.golden_util import Golden, full_cfg, tiny_cfg
from tests.test_att_apply_args_cpu import _caller
from tests.test_feature_train_cpu import _fake_feats


def test_drop_then_normalise_of_the_cached_features_is_the_reference_order():
    """pooled [3, 5, 16] post-ReLU-like (about half the entries zero), keep-masks at p = 0.3.  Wherever the kept part of a row has
    norm >= 1e-3 the two orders agree to 1e-9 relative; a row whose kept part is all zero gives exact zeros, no NaN, in both."""
    g = torch.Generator().manual_seed(20)
    pooled = torch.relu(torch.randn(3, 5, 16, generator=g, dtype=torch.float64))
    keep = lambda: (torch.rand(3, 5, 16, generator=g) >= 0.3).double() / 0.7
    mask_img, mask_att = keep(), keep()
    pooled[0, 1] *= (mask_img[0, 1] == 0)                  # rows whose kept part is all zero: one that is not zero itself,
    pooled[2, 4] = 0                                       # and one that is
    assert float(pooled[0, 1].abs().max()) > 0
    zero_frac = float((pooled == 0).double().mean())
    assert 0.35 < zero_frac < 0.65, zero_frac
    rows = torch.tensor([2, 0, 2, 1])
    kept = kept_norms(pooled, rows, mask_img)
    dead, live = kept == 0, kept >= 1e-3
    assert bool((dead | live).all()) and int(dead.sum()) >= 3 and int(live.sum()) >= 10        # both kinds of row, nothing between
    vn, vdrop = drop_norm(l2norm(pooled), rows, mask_img, mask_att)
    want = oracle_drop_then_norm(pooled, mask_img)[rows]
    assert not bool(torch.isnan(vn).any()) and not bool(torch.isnan(want).any())
    assert bool((vn[dead] == 0).all()) and bool((want[dead] == 0).all()) and bool((vdrop[dead] == 0).all())
    err = (vn - want).abs()[live]
    assert bool((err <= 1e-9 * want.abs()[live]).all()), float(err.max())
    assert float((vn[live].norm(dim=-1) - 1).abs().max()) < 1e-9                               # renormalised rows
    assert torch.equal(vdrop, vn * mask_att[rows])
    assert torch.equal(drop_norm(l2norm(pooled), rows, mask_img), vn)
    # an out-of-range entry: zeros in both outputs
    a, b = drop_norm(l2norm(pooled), [1, 3, -1], mask_img, mask_att)
    assert float(a[1:].abs().max()) == 0 and float(b[1:].abs().max()) == 0 and float(a[0].abs().max()) > 0


NAMES = ("src", "rows", "vn_out", "vdrop_out", "n", "M", "P", "C", "p", "seed", "p2", "seed2", "stream")


@pytest.mark.parametrize("entry,src_align", [("vqa_gather_rows_drop_norm", 16), ("vqa_gather_rows_drop_norm_f16", 8)])
def test_gather_rows_drop_norm_argument_validation_without_gpu(entry, src_align):
    from dl_vqa_amd import _lib
    lib = _lib.load()
    err = lib.vqa_last_error
    call = _caller(getattr(lib, entry), NAMES, (64, 64, 64, 64, 3, 5, 7, 8, 0.3, 1, 0.3, 2, None))
    for name in ("src", "rows", "vn_out"):
        assert call(**{name: None}) == 1 and b"null pointer" in err() and entry.encode() + b":" in err(), name
    assert call(C=6) == 1 and b"C=6" in err()
    assert call(C=0) == 1 and b"C=0" in err()
    assert call(P=0) == 1 and b"out of range" in err()
    assert call(M=0) == 1 and b"out of range" in err()
    assert call(n=-1) == 1 and b"out of range" in err()
    assert call(p=1.0) == 1 and b"p=1" in err()
    assert call(p2=1.0) == 1 and b"p2=1" in err()
    assert call(p=-0.1) == 1 and call(p2=-0.1) == 1
    assert call(src=64 + src_align // 2) == 1 and b"src must be" in err() and b"aligned" in err()
    if src_align == 8:
        assert call(src=64 + 8, n=0) == 0                           # a half bank: 8 bytes are enough
    for name in ("vn_out", "vdrop_out"):
        assert call(**{name: 64 + 8}) == 1 and b"16-byte aligned" in err(), name
    assert call(n=0) == 0                                           # no launch
    assert call(n=0, vdrop_out=None) == 0                           # optional
    assert call(n=0, vdrop_out=None, p2=1.0) == 0                   # ... and p2 is then ignored
    assert call(n=0, C=6) == 1                                      # the checks come before the early return


def test_new_entry_points_are_additions_and_the_abi_version_stays():
    """Added without a version bump: bound last in _lib.PROTOTYPES, declared in the header (with the entry points of training
    on cached image features: tests/test_half_features_cpu.py pins what the header ends with), listed in the comment that
    records the additions, exported by the library."""
    import re
    from dl_vqa_amd import _lib
    new = ["vqa_gather_rows_drop_norm", "vqa_gather_rows_drop_norm_f16"]
    assert list(_lib.PROTOTYPES)[-2:] == new
    assert _lib.header_abi_version() == 9 and _lib.load().vqa_abi_version() == 9
    with open(_lib.HEADER_PATH) as f:
        text = f.read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in new:
        assert len(re.findall(r"\bint " + name + r"\s*\(", code)) == 1, name
        assert name in text.split("#define VQA_ABI_VERSION")[0], name
        assert hasattr(_lib.load(), name), name


@pytest.mark.parametrize("bad", [1, 0, "yes", None, 1.0])
def test_image_dropout_must_be_a_bool_before_any_device_work(bad):
    from dl_vqa_amd.train import run_batch_features
    g = Golden("tiny_plus")
    m = VqaNet(tiny_cfg(g.meta), g.meta["V"])                       # on the CPU
    q, ql = torch.ones(2, 3, dtype=torch.int64), torch.tensor([3, 3])
    feats = _fake_feats(torch.zeros(1, 4, 8))
    with pytest.raises(ValueError, match="image_dropout must be a bool"):
        m.forward_features(feats, q, ql, [0, 0], image_dropout=bad)
    with pytest.raises(ValueError, match="image_dropout must be a bool"):
        m.forward_features(None, q, ql, [0, 0], bad)                # before feats is looked at
    batch = (None, g.t["q"], g.t["a_idx"], g.t["a_val"], g.t["a_len"], torch.arange(3), g.t["q_len"])
    with pytest.raises(ValueError, match="image_dropout must be a bool"):
        run_batch_features(m, batch, 12, feats, [0, 0, 0], image_dropout=bad)
    assert m._last_ctx is None and m._flat_param is None and len(m._pending) == 0


def test_a_bool_reaches_the_checks_that_were_there():
    """True and False pass the new check: bf16 and a data-parallel model still raise NotImplementedError, a CPU model the
    device error."""
    q, ql = torch.ones(2, 3, dtype=torch.int64), torch.tensor([3, 3])
    feats = _fake_feats(torch.zeros(1, 4, 256))
    m = VqaNet(full_cfg(16), 30, compute_dtype="bf16")
    g = Golden("tiny_plus")
    t = VqaNet(tiny_cfg(g.meta), g.meta["V"])
    for flag in (True, False):
        with pytest.raises(NotImplementedError, match="compute_dtype"):
            m.forward_features(feats, q, ql, [0, 0], image_dropout=flag)
        t._grad_sync = object()
        with pytest.raises(NotImplementedError, match="data-parallel"):
            t.forward_features(feats, q, ql, [0, 0], image_dropout=flag)
        t._grad_sync = None
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            t.forward_features(feats, q, ql, [0, 0], image_dropout=flag)
