"""tests/step_links.py held to itself, without a GPU: its float64 reference against a plain torch float64 matmul in every layout
and epilogue form the engine uses, an honest stand-in step that must pass every link well inside its bound (the CPU check of
the tolerance), and wrong stand-ins (nine, and a pad of -0) that audit() must each report.

The stand-ins take the place of dl_vqa_amd.engine / dl_vqa_amd.ops for the Recorder: the same entry points with the same
arguments, computed by torch on the CPU -- fp32 products of bf16-valued operands, the epilogue in epi_apply's order, bf16 copies
by round-to-nearest-even."""
from types import SimpleNamespace

import pytest
import torch

from tests import step_links as L
from tests.test_streaming_gpu import tol_sum

BF = torch.bfloat16
SLACK = 4096        # elements behind every stand-in buffer: a wrong leading dimension reads them instead of leaving the storage


def alloc(rows, cols, dtype=torch.float32, ld=None):
    ld = cols if ld is None else ld
    flat = torch.zeros(rows * ld + SLACK, dtype=dtype)
    return flat[:rows * ld].view(rows, ld)[:, :cols]


def rand(g, rows, cols, ld=None, bf16_valued=False, dtype=torch.float32):
    """a random [rows][cols] matrix with leading dimension ld; the gap and the slack hold other random values"""
    ld = cols if ld is None else ld
    flat = torch.randn(rows * ld + SLACK, generator=g)
    if bf16_valued or dtype == BF:
        flat = flat.to(BF).to(dtype)
    return flat[:rows * ld].view(rows, ld)[:, :cols]


def standin(mutant=None):
    """(engine, ops) stand-ins; mutant: one of MUTANTS, or None for the honest step"""
    ops = SimpleNamespace()

    def to_bf16(x, out=None):
        y = out if out is not None else alloc(1, x.numel(), BF).view(x.shape)
        r = (x.contiguous().view(torch.int32) & -65536).view(torch.float32) if mutant == "truncation" else x
        y.copy_(r.to(BF).view(y.shape))
        return y

    def add2d(a, lda, b, ldb, out, ldo, rows, cols):
        src = L._view(a, rows, cols, ldo if (mutant == "narrowing stride" and ldo < lda) else lda)
        L._view(out, rows, cols, ldo).copy_(src if b is None else src + L._view(b, rows, cols, ldb))
        return out

    def product(A, B, C, M, N, K, transA=False, transB=True, lda=None, ldb=None, ldc=None, bias1=None, bias2=None, rowgroup=None,
                rg_div=1, rg_op=0, relu=False, accumulate=False, aux=None, tag=0):
        lda = lda if lda is not None else (M if transA else K)
        ldb = ldb if ldb is not None else (K if transB else N)
        ldc = ldc if ldc is not None else N
        Ke = K - 8 if mutant == "K tail dropped" and K > 8 else K
        a = L._view(A, M, K, lda, transA).float()
        b = L._view(B, K, N, ldb + (mutant == "ldb off by one"), transB).float()
        v = a[:, :Ke] @ b[:Ke]
        if aux is not None:
            L._view(aux, M, N, ldc).copy_(v)
        if rowgroup is not None:
            div = rg_div + (mutant == "row group divisor")
            g = L._view(rowgroup, -(-M // rg_div), N, rowgroup.stride(0))[torch.arange(M) // div]
            v = v * g if rg_op else v + g
        if relu and mutant == "ReLU before bias":
            v = torch.clamp_min(v, 0.0)
        for bias in (bias1, bias2):
            if bias is not None:
                v = v + bias
        if relu and mutant != "ReLU before bias":
            v = torch.clamp_min(v, 0.0)
        c = L._view(C, M, N, ldc)
        if accumulate and mutant != "accumulate ignored":
            v = v + c
        c.copy_(v.to(C.dtype))
        return C

    ops.to_bf16, ops.add2d = to_bf16, add2d
    ops.gemm_tall_bf16 = lambda A, W, C, M, N, K, **kw: product(A, W, C, M, N, K, lda=A.stride(0), ldb=W.stride(0), ldc=C.stride(0), **kw)
    ops.gemm_plan = lambda engine, M, N, K, **kw: dict(BM=64, BN=64, splits=1, persistent=0, wide=0)
    ops.gemm_tall_bf16_plan = lambda M, N, K: dict(BM=256, grid=1, nk=K // 64)

    class Engine:
        @staticmethod
        def _rows16(x, ld, rows, cols, rows8):
            t = alloc(rows, cols)
            ops.add2d(x, ld, None, 0, t, cols, rows, cols)
            out = alloc(rows8, cols, BF)
            ops.to_bf16(t, out=out[:rows])
            if mutant == "rows16 pad row" and rows8 > rows:
                out[rows, 1] = 1e-30
            return out

        @staticmethod
        def _cols16(x, rows, cols, cols8):
            t = alloc(rows, cols8)
            ops.add2d(x.reshape(rows, cols), cols, None, 0, t, cols8, rows, cols)
            out = ops.to_bf16(t)
            if mutant in ("cols16 pad column", "cols16 pad minus zero") and cols8 > cols:
                out[2, cols] = 1e-30 if mutant == "cols16 pad column" else -0.0
            return out

    engine = SimpleNamespace(Engine=Engine, _gemm=lambda A, B, C, M, N, K, x3=False, **kw: product(A, B, C, M, N, K, **kw))
    return engine, ops


def standin_step(eng, ops, do_option="+", bf16=True, seed=3):
    """The step's chain of casts and products in the engine's call forms and order, at toy widths: B = 3 rows padded to 8,
    B * Pn = 24, E = 20 -> 24, T * B = 16.  bf16: the bf16 forms; otherwise the fp32 forms (bf16-valued fp32 operands), q_lin's
    dq accumulated into dcomb's question columns with ldc = Dc."""
    g = torch.Generator().manual_seed(seed)
    B, B8, Pn, C, mid, Q, GC, hid, A = 3, 8, 8, 16, 24, 16, 32, 24, 16
    TB, E, Ek, H4, H = 16, 20, 24, 32, 8
    Dc, mode = GC + Q, {"+": 0, "*": 1, "|": 2}[do_option]
    Eng = eng.Engine
    w = lambda r, c: rand(g, r, c, bf16_valued=not bf16)        # fp32 parameters / activations (fp32 forms: bf16-valued)
    fc = lambda x, ld, cols: Eng._rows16(x, ld, B, cols, B8) if bf16 else x
    wt = lambda x: ops.to_bf16(x.contiguous()) if bf16 else x
    Bk = B8 if bf16 else B
    # ---- forward
    x_emb, w_ih = w(TB, E), w(H4, E)
    Ekk = Ek if bf16 else E
    x_op, wih_op = (Eng._cols16(x_emb, TB, E, Ek), Eng._cols16(w_ih, H4, E, Ek)) if bf16 else (x_emb, w_ih)
    xg = alloc(TB, H4)
    eng._gemm(x_op, wih_op, xg, TB, H4, Ekk, bias1=w(1, H4)[0], bias2=w(1, H4)[0], tag=10)
    combined = w(B, Dc)
    wq, w1, w2, wv = wt(w(mid, Q)), wt(w(hid, Dc)), wt(w(A, hid)), wt(w(mid, C))
    q_op = fc(combined[:, GC:], Dc, Q)
    qp = alloc(B, mid)
    eng._gemm(q_op, wq, qp, B, mid, Q, lda=Q if bf16 else Dc, bias1=w(1, mid)[0], tag=20)
    v_op = wt(w(B * Pn, C))
    xs = alloc(B * Pn, mid, BF if bf16 else torch.float32)
    vprime = alloc(B * Pn, mid) if mode == 1 else None
    epi = dict(rowgroup=(qp if mode != 2 else None), rg_div=Pn, rg_op=(1 if mode == 1 else 0), relu=True, tag=21)
    if bf16 and vprime is None:
        ops.gemm_tall_bf16(v_op, wv, xs, B * Pn, mid, C, **epi)
    else:
        eng._gemm(v_op, wv, xs, B * Pn, mid, C, aux=vprime, **epi)
    c_op = fc(combined, Dc, Dc)
    h1, logits = alloc(B, hid), alloc(B, A)
    eng._gemm(c_op, w1, h1, B, hid, Dc, bias1=w(1, hid)[0], relu=True, tag=30)
    h_op = fc(h1, hid, hid)
    eng._gemm(h_op, w2, logits, B, A, hid, bias1=w(1, A)[0], tag=31)
    # ---- backward
    dlogits = w(B, A)
    dl_op = fc(dlogits, A, A)
    dw2, dh1, dw1, dcomb = alloc(A, hid), alloc(B, hid), alloc(hid, Dc), alloc(B, Dc)
    eng._gemm(dl_op, h_op, dw2, A, hid, Bk, transA=True, transB=False, lda=A, ldb=hid, tag=40)
    eng._gemm(dl_op, w2, dh1, B, hid, A, transB=False, lda=A, ldb=hid, tag=41)
    dh_op = fc(dh1, hid, hid)
    eng._gemm(dh_op, c_op, dw1, hid, Dc, Bk, transA=True, transB=False, lda=hid, ldb=Dc, tag=42)
    eng._gemm(dh_op, w1, dcomb, B, Dc, hid, transB=False, lda=hid, ldb=Dc, tag=43)
    dxpre = xs
    dxpre.copy_(rand(g, B * Pn, mid, bf16_valued=True))            # overwritten in place, as att_score_bwd does
    dwv, dv_in = alloc(mid, C), alloc(B * Pn, C)
    eng._gemm(dxpre, v_op, dwv, mid, C, B * Pn, transA=True, transB=False, lda=mid, ldb=C, tag=44)
    eng._gemm(dxpre, wv, dv_in, B * Pn, C, mid, transB=False, lda=mid, ldb=C, tag=45)
    dqp = w(B, mid)
    dqp_op = fc(dqp, mid, mid)
    dwq = alloc(mid, Q)
    eng._gemm(dqp_op, q_op, dwq, mid, Q, Bk, transA=True, transB=False, lda=mid, ldb=Q if bf16 else Dc, tag=46)
    dq_in, ld_dq = (alloc(B, Q), Q) if bf16 else (dcomb[:, GC:], Dc)
    eng._gemm(dqp_op, wq, dq_in, B, Q, mid, transB=False, lda=mid, ldb=Q, ldc=ld_dq, accumulate=not bf16, tag=47)
    dgates, h_in = w(TB, H4), w(TB, H)
    dg_op, hh_op = wt(dgates), wt(h_in)
    dw_hh, dw_ih, dx = alloc(H4, H), alloc(H4, E), alloc(TB, E)
    eng._gemm(dg_op, hh_op, dw_hh, H4, H, TB, transA=True, transB=False, lda=H4, ldb=H, tag=51)
    dwp = dw_ih if Ekk == E else alloc(H4, Ekk)
    eng._gemm(dg_op, x_op, dwp, H4, Ekk, TB, transA=True, transB=False, lda=H4, ldb=Ekk, tag=52)
    if Ekk != E:
        ops.add2d(dwp, Ekk, None, 0, dw_ih, E, H4, E)
    dxp = dx if Ekk == E else alloc(TB, Ekk)
    eng._gemm(dg_op, wih_op, dxp, TB, Ekk, H4, transB=False, lda=H4, ldb=Ekk, tag=53)
    if Ekk != E:
        ops.add2d(dxp, Ekk, None, 0, dx, E, TB, E)


def half_ulp_bf16(x):
    """half the distance between neighbouring bf16 values at |x| = m 2^e, m in [0.5, 1): 2^(e - 9); 0 at 0"""
    e = torch.frexp(x)[1]
    return torch.where(x == 0, torch.zeros_like(x), torch.ldexp(torch.ones_like(x), e - 9))


TAGS = [10, 20, 21, 30, 31, 40, 41, 42, 43, 44, 45, 46, 47, 51, 52, 53]


def record(mutant=None, **kw):
    eng, ops = standin(mutant)
    with L.Recorder(eng, ops) as rec:
        standin_step(eng, ops, **kw)
    return rec.links


# ------------------------------------------------------------------------------------------------ the reference
# every epilogue combination the engine uses, by tag: (bias vectors, row-group op or None, ReLU, accumulate, aux, bf16 C)
EPILOGUES = {"10": (2, None, False, False, False, False), "20": (1, None, False, False, False, False),
             "21+": (0, 0, True, False, False, True), "21*": (0, 1, True, False, True, True), "21|": (0, None, True, False, False, True),
             "21+ fp32": (0, 0, True, False, False, False), "21* fp32": (0, 1, True, False, True, False),
             "30": (1, None, True, False, False, False), "31": (1, None, False, False, False, False),
             "40-46, 51-53": (0, None, False, False, False, False), "47": (0, None, False, True, False, False)}


@pytest.mark.parametrize("name", list(EPILOGUES))
@pytest.mark.parametrize("transA,transB", [(False, True), (False, False), (True, True), (True, False)])
def test_product_ref_is_the_float64_matmul(name, transA, transB):
    """Dense A [M][K] and B [K][N] stored in each of the four layouts with leading dimensions longer than the rows (other random
    values in the gaps), C and aux with ldc > N: the recorded op(A), op(B) are the dense matrices, and product_ref is torch's
    float64 matmul followed by the epilogue written out here."""
    nbias, rg_op, relu, accumulate, has_aux, c_bf16 = EPILOGUES[name]
    M, N, K, rg_div = 21, 10, 13, 7
    g = torch.Generator().manual_seed(len(name) * 4 + 2 * transA + transB)
    Ad, Bd = torch.randn(M, K, generator=g).to(BF), torch.randn(K, N, generator=g).to(BF)
    lda, ldb, ldc = (M if transA else K) + 5, (K if transB else N) + 3, N + 6
    A = rand(g, *((K, M) if transA else (M, K)), ld=lda, dtype=BF)
    B = rand(g, *((N, K) if transB else (K, N)), ld=ldb, dtype=BF)
    A.copy_(Ad.t() if transA else Ad)
    B.copy_(Bd.t() if transB else Bd)
    C = rand(g, M, N, ld=ldc, dtype=BF if c_bf16 else torch.float32)
    C0 = C.clone()
    aux = rand(g, M, N, ld=ldc) if has_aux else None
    b1, b2 = (torch.randn(N, generator=g) if nbias >= 1 else None), (torch.randn(N, generator=g) if nbias >= 2 else None)
    rgt = rand(g, M // rg_div, N, ld=N + 4) if rg_op is not None else None
    eng, ops = standin()
    with L.Recorder(eng, ops) as rec:
        eng._gemm(A, B, C, M, N, K, transA=transA, transB=transB, lda=lda, ldb=ldb, ldc=ldc, bias1=b1, bias2=b2, rowgroup=rgt,
                  rg_div=rg_div, rg_op=rg_op or 0, relu=relu, accumulate=accumulate, aux=aux, tag=7)
    (link,) = rec.links
    assert torch.equal(link.A, Ad) and torch.equal(link.B, Bd)
    assert (link.lda, link.ldb, link.ldc, link.transA, link.transB, link.tag) == (lda, ldb, ldc, transA, transB, 7)
    prod = Ad.double() @ Bd.double()
    want = prod
    if rg_op is not None:
        rows = rgt.double().repeat_interleave(rg_div, dim=0)
        want = want * rows if rg_op else want + rows
    if b1 is not None:
        want = want + b1.double()
    if b2 is not None:
        want = want + b2.double()
    if relu:
        want = torch.relu(want)
    if accumulate:
        want = want + C0.double()
    got_prod, got = L.product_ref(link)
    assert torch.allclose(got_prod, prod, rtol=0, atol=1e-13) and torch.allclose(got, want, rtol=0, atol=1e-13)
    assert (link.C0 is not None) == accumulate and (link.aux is not None) == has_aux
    assert L.audit(rec.links, check=False) == []


# ------------------------------------------------------------------------------------------------ the honest step
@pytest.mark.parametrize("do_option,bf16", [("+", True), ("*", True), ("|", True), ("+", False), ("*", False), ("|", False)])
def test_honest_step_passes_inside_a_quarter_of_the_bound(do_option, bf16):
    """fp32 torch products of bf16-valued operands: every fp32 result within 0.25 of tol_sum(K + 3) -- the CPU check of the
    tolerance.  A bf16 result carries its own rounding on top, up to half a bf16 ulp of the element (2^-8 |ref| at the low end of
    a binade: the whole first term of check_bf16): what is left of its error after half an ulp is taken off must stay within
    0.25 T max|ref| as well.  Casts and copies: no bit differs."""
    links = record(do_option=do_option, bf16=bf16)
    assert [l.tag for l in L.products(links)] == TAGS
    assert L.audit(links) == []
    for l in links:
        _, err, bound, _ = L.judge(l)
        if l.kind == "product":
            assert bound == (1.0 if l.C.dtype == BF else tol_sum(l.K + 3))
            if l.C.dtype == BF:
                assert err <= 1.0
                ref, got = L.product_ref(l)[1], l.C.double()
                err, bound = float((((got - ref).abs() - half_ulp_bf16(torch.maximum(got.abs(), ref.abs()))).clamp_min(0)).max()
                                   / ref.abs().max()), tol_sum(l.K + 3)
            assert err <= 0.25 * bound, (l.tag, l.K, err, bound)
        else:
            assert err == 0.0
    if bf16:
        assert {c.name for c in L.casts(links)} == {"to_bf16", "_rows16", "_cols16"}
        assert [(c.rows, c.rows8) for c in L.casts(links, "_rows16")][0] == (3, 8)
        assert [(c.cols, c.cols8) for c in L.casts(links, "_cols16")][0] == (20, 24)
        tall = [l for l in L.products(links, 21) if l.engine == L.TALL]
        assert len(tall) == (do_option != "*")
        p52, p53 = L.products(links, 52)[0], L.products(links, 53)[0]
        assert L.narrowing(links, p52).cols == 20 and L.narrowing(links, p53).ldo == 20
    else:
        (p47,) = L.products(links, 47)
        assert p47.accumulate and p47.C0 is not None and p47.ldc == 48 and not L.casts(links)


# ------------------------------------------------------------------------------------------------ the mutants
# name -> (stand-in flavour that reaches it, which report shows it)
MUTANTS = {
    "K tail dropped": (dict(), lambda f: "tag 10" in f and "max|got - ref|" in f),
    "ldb off by one": (dict(), lambda f: "tag 20" in f),
    "truncation": (dict(), lambda f: "cast to_bf16" in f and "round-to-nearest-even" in f),
    "cols16 pad column": (dict(), lambda f: "cast _cols16" in f and "pad elements are not +0" in f),
    "rows16 pad row": (dict(), lambda f: "cast _rows16" in f and "pad elements are not +0" in f),
    "cols16 pad minus zero": (dict(), lambda f: "cast _cols16" in f and "pad elements are not +0" in f),     # beyond the nine: +0 means +0
    "ReLU before bias": (dict(), lambda f: "tag 30" in f),
    "accumulate ignored": (dict(bf16=False), lambda f: "tag 47" in f),
    "row group divisor": (dict(do_option="*"), lambda f: "tag 21" in f),
    "narrowing stride": (dict(), lambda f: "copy add2d" in f and "ld 24 -> 20" in f),
}


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_audit_reports_the_mutant(mutant):
    """Each wrong stand-in is reported by audit(), by the link it breaks; the honest stand-in of the same flavour is not."""
    kw, shows = MUTANTS[mutant]
    assert L.audit(record(**kw), check=False) == []
    failures = L.audit(record(mutant, **kw), check=False)
    assert any(shows(f) for f in failures), f"mutant '{mutant}' was not reported: {failures}"
    with pytest.raises(AssertionError, match="link finding"):
        L.audit(record(mutant, **kw))


def test_every_mutant_of_the_issue_is_listed():
    assert set(MUTANTS) >= {"K tail dropped", "ldb off by one", "truncation", "cols16 pad column", "rows16 pad row",
                            "ReLU before bias", "accumulate ignored", "row group divisor", "narrowing stride"}
