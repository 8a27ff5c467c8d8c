"""The train step outside the conv blocks at the north-star widths, link by link (tests/step_links.py): every dense product the
step launches against float64 on the operands the device held, every bf16 copy bit for bit against round-to-nearest-even.

Each case is one forward + one backward of VqaNet on tests.golden_util.full_cfg(1000) -- E = 300, H = 1024 bidirectional,
mid = hid = 1024, G = 2, C = 256, A = 1000 -- with V = 3000, seeded weights, small images, ragged q_len that includes 1 and T,
and a seeded random dlogits (144 px: the bf16 path's first block takes image widths that are multiples of 4).  What only
that case reaches is asserted before the audit:

  a  bf16 train '+'      B 8, 144 px (P 256), T 3   vqa_gemm_tall_bf16 2048 x 1024 x 256, rg_div 256, 64 tiles (its minimum);
                                                    FC rows need no padding; lstm16 with K = T B = 24
  b  bf16 train + * |    B 4,  68 px (P 36), T 14   v_conv on vqa_gemm_bf16 with rg_div 36 < tile height (general row-group
                                                    epilogue), '*': the fp32 aux out of the bf16 GEMM; FC rows 4 -> 8; lstm16
                                                    with T B = 56, E 300 -> 304 (N = 304 edge tiles)
  c  bf16 train '+'      B 2,  68 px (P 36), T 14   T B = 28: the LSTM-side products fall back to fp32 inside bf16 mode
  d  bf16 train '+'      B 3,  68 px (P 36), T 8    B P = 108 = 4 (mod 8): the v_conv weight gradient's K is no multiple of 8;
                                                    FC rows 3 -> 8; lstm16 with T B = 24
  e  fp32 train + * |    B 4,  68 px (P 36), T 14   the same products on vqa_gemm, the fp32 row-group forms included
  f  fp32 eval  '+'      B 3,  68 px (P 36), T 8    p_att = 0: q_lin's dq accumulates straight into dcomb[:, GC:] (ldc = Dc)
"""
import pytest
import torch

from tests import step_links as L
from tests.step_links import BF16, F32, TALL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
V, A, E, EK, H, MID, C, GC, DC = 3000, 1000, 300, 304, 1024, 1024, 256, 512, 2560

CASES = {
    "a": dict(dtype="bf16", train=True, mode="+", B=8, S=144, P=256, T=3),
    "b+": dict(dtype="bf16", train=True, mode="+", B=4, S=68, P=36, T=14),
    "b*": dict(dtype="bf16", train=True, mode="*", B=4, S=68, P=36, T=14),
    "b|": dict(dtype="bf16", train=True, mode="|", B=4, S=68, P=36, T=14),
    "c": dict(dtype="bf16", train=True, mode="+", B=2, S=68, P=36, T=14),
    "d": dict(dtype="bf16", train=True, mode="+", B=3, S=68, P=36, T=8),
    "e+": dict(dtype="fp32", train=True, mode="+", B=4, S=68, P=36, T=14),
    "e*": dict(dtype="fp32", train=True, mode="*", B=4, S=68, P=36, T=14),
    "e|": dict(dtype="fp32", train=True, mode="|", B=4, S=68, P=36, T=14),
    "f": dict(dtype="fp32", train=False, mode="+", B=3, S=68, P=36, T=8),
}

# The products of one step in launch order, and the engine each runs on, per case.  Columns: the LSTM-side products (10, 51-53),
# the batch-row FC products (20, 30, 31, 40-43, 46, 47), v_conv forward (21), its two gradients (44, 45).  Case d alone has a
# second tag-44 launch: the last B P mod 8 rows of the weight gradient, accumulated by the fp32 GEMM.
ORDER = [10, 10, 20, 21, 30, 31, 40, 41, 42, 43, 44, 45, 46, 47, 51, 52, 53, 51, 52, 53]
ENGINES = {          # lstm, fc, v_conv forward, v_conv gradients
    "a": (BF16, BF16, TALL, BF16), "b+": (BF16, BF16, BF16, BF16), "b*": (BF16, BF16, BF16, BF16), "b|": (BF16, BF16, BF16, BF16),
    "c": (F32, BF16, BF16, BF16), "d": (BF16, BF16, BF16, BF16),
    "e+": (F32, F32, F32, F32), "e*": (F32, F32, F32, F32), "e|": (F32, F32, F32, F32), "f": (F32, F32, F32, F32),
}


def tag_table(case):
    lstm, fc, fwd, grad = ENGINES[case]
    col = {10: lstm, 51: lstm, 52: lstm, 53: lstm, 21: fwd, 44: grad, 45: grad}
    out = []
    for tag in ORDER:
        out.append((tag, col.get(tag, fc)))
        if tag == 44 and case == "d":
            out.append((44, F32))
    return out


def run_case(case):
    """(model, ctx, links) of the case's recorded forward + backward"""
    from dl_vqa_amd import VqaNet
    from oracle import vqa_oracle as O
    from tests.golden_util import full_cfg
    c = CASES[case]
    B, S, T = c["B"], c["S"], c["T"]
    cfg = full_cfg(A)
    cfg["attention"]["do_option"] = c["mode"]
    torch.manual_seed(20 + len(case) + B)
    m = VqaNet(cfg, V, compute_dtype=c["dtype"]).to(DEV)
    m.train(c["train"])
    v, q, *_ = O.synthetic_batch(B, S, T, V, A, seed=30 + B, full_len=True)
    q_len = torch.tensor([1, T] + [1 + (3 * i) % T for i in range(B - 2)], dtype=torch.int64)      # ragged, 1 and T included
    q = q * (torch.arange(T)[None, :] < q_len[:, None])
    g = torch.Generator().manual_seed(40 + B)
    dlogits = torch.randn(B, A, generator=g).to(DEV)
    torch.manual_seed(9)
    with L.Recorder() as rec:
        y = m(v.to(DEV), q.to(DEV), q_len.to(DEV))
        y.backward(dlogits)
        torch.cuda.synchronize()
    return m, m._last_ctx, rec.links


@pytest.mark.parametrize("case", list(CASES))
def test_step_links(case):
    c = CASES[case]
    B, P, T = c["B"], c["P"], c["T"]
    bf16, mode = c["dtype"] == "bf16", c["mode"]
    m, ctx, links = run_case(case)
    prods = L.products(links)
    # ---- the case reached what it is listed for
    assert ctx.Pn == P
    assert [(l.tag, l.engine) for l in prods] == tag_table(case)
    l16 = bf16 and (T * B) % 8 == 0
    assert l16 == (case in ("a", "b+", "b*", "b|", "d"))
    if l16:
        assert ctx.x16 is not None and tuple(ctx.x16.shape) == (T * B, EK) and ctx.x16.dtype == torch.bfloat16
        assert [(l.M, l.N, l.K) for l in L.products(links, 10, 52, 53)] == \
            2 * [(T * B, 4 * H, EK)] + 2 * [(4 * H, EK, T * B), (T * B, EK, 4 * H)]
        assert [(x.rows, x.cols, x.cols8) for x in L.casts(links, "_cols16")] == [(T * B, E, EK), (4 * H, E, EK), (4 * H, E, EK)]
    else:
        assert ctx.x16 is None and not L.casts(links, "_cols16")
    assert (ctx.fc is not None) == bf16
    rows16 = L.casts(links, "_rows16")
    if bf16:
        assert len(rows16) == 6 and all((x.rows, x.rows8) == (B, (B + 7) // 8 * 8) for x in rows16)
        assert [l.K for l in L.products(links, 40, 42, 46)] == 3 * [(B + 7) // 8 * 8]
    else:
        assert not L.casts(links)
    (fwd,) = L.products(links, 21)
    assert (fwd.M, fwd.N, fwd.K, fwd.rg_div) == (B * P, MID, C, P)
    assert (fwd.rowgroup is not None) == (mode != "|") and fwd.rg_op == (mode == "*") and fwd.relu
    assert (fwd.aux is not None) == (mode == "*") and (fwd.aux is None or fwd.aux.dtype == torch.float32)
    assert fwd.C.dtype == (torch.bfloat16 if bf16 else torch.float32)
    assert (fwd.engine == TALL) == (case == "a")
    if case == "a":
        assert (fwd.M, fwd.rg_div, fwd.plan["tiles_m"] * fwd.plan["tiles_n"]) == (2048, 256, 64)
    if case.startswith("b"):
        assert fwd.rg_div == 36 < fwd.plan["BM"]
    dwv = L.products(links, 44)
    if case == "d":
        assert (B * P) % 8 == 4 and [(l.K, l.accumulate, l.C0 is not None) for l in dwv] == [(104, False, False), (4, True, True)]
    else:
        assert [(l.K, l.accumulate) for l in dwv] == [(B * P, False)]
    (dq,) = L.products(links, 47)
    assert (dq.accumulate, dq.ldc, dq.C0 is not None) == ((True, DC, True) if case == "f" else (False, 2 * H, False))
    # ---- every link
    L.audit(links, label=f"{case:2s} ")
    # ---- the Ek -> E narrowing copies and the zero pad columns, exactly
    if l16:
        grads = dict(m.named_parameters())
        for d, (dw, dx) in enumerate(zip(L.products(links, 52), L.products(links, 53))):
            cw, cx = L.narrowing(links, dw), L.narrowing(links, dx)
            assert (cw.rows, cw.cols, cw.lda, cw.ldo) == (4 * H, E, EK, E) and (cx.rows, cx.cols, cx.lda, cx.ldo) == (T * B, E, EK, E)
            assert torch.equal(cw.out, dw.C[:, :E]) and torch.equal(cx.out, dx.C[:, :E])
            assert torch.equal(grads["text.lstm.weight_ih_l0" + ("_reverse" if d else "")].grad, dw.C[:, :E])
            assert bool((dw.C[:, E:] == 0).all()) and bool((dx.C[:, E:] == 0).all())     # sums of products with a zero pad column
