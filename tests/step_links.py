"""The train step outside the conv blocks as a chain of links, each held against the operands the device actually held.

A Recorder wraps the five places through which the step launches a dense product or makes a bf16 copy -- engine._gemm,
ops.gemm_tall_bf16, ops.to_bf16, Engine._rows16, Engine._cols16 -- and the plain strided copies of ops.add2d (the Ek -> E
narrowing copies of the LSTM-side products are such copies).  It changes no product code (pytest.MonkeyPatch only) and
records, per call, clones of what the call read and of what it wrote, taken on the stream the call ran on: the recorded step
runs with VQA_STREAMS=0, one stream, so every clone is ordered between the launch before it and the launch after it.

  product  C = epi(op(A) op(B)): op(A) [M][K] and op(B) [K][N] read back through the pointer, leading dimension and transpose
           flag the call passed, in the type they have; bias, row-group, aux; C before the call when it accumulates; C and aux
           after it.  product_ref: float64 on those operands, the epilogue as epi_apply (csrc/gemm_epilogue.hpp).  A product
           of two bf16 values is exact in fp32, so the kernel's whole error is its fp32 accumulation: an fp32 result (and aux)
           must satisfy max|got - ref| / max|ref| <= tol_sum(K + 3), a bf16 result check_bf16 with T = tol_sum(K + 3) (both
           from tests/test_streaming_gpu.py), no element exempt.
  cast     a bf16 copy: element for element the round-to-nearest-even of the fp32 tensor it was made from (torch.equal's
           equality: Engine._cols16 stages through add2d, whose a + 0 turns a -0 of the source into +0); pad rows / columns
           +0, bit for bit.
  copy     out[r, c] = a[r, c] between two leading dimensions, element for element (the same equality).

No GPU import at module level: the targets default to dl_vqa_amd.engine / dl_vqa_amd.ops and are imported on entry; the CPU
test hands in stand-ins of its own.
"""
from types import SimpleNamespace

import pytest
import torch

from tests.test_streaming_gpu import check_bf16, tol_sum

F32, X3, BF16, TALL = "vqa_gemm", "vqa_gemm_x3", "vqa_gemm_bf16", "vqa_gemm_tall_bf16"


def _view(t, rows, cols, ld, transposed=False):
    """[rows][cols] as the kernels address it from t's first element: element (r, c) at r * ld + c, or -- transposed, a stored
    [cols][rows] matrix -- at c * ld + r.  as_strided refuses a view that leaves the storage."""
    return t.as_strided((rows, cols), (1, ld) if transposed else (ld, 1), t.storage_offset())


def _clone(t):
    return None if t is None else t.detach().clone()


class Recorder:
    """with Recorder() as rec: one forward + backward; rec.links then holds every link in launch order."""

    def __init__(self, engine=None, ops=None):
        self.engine, self.ops = engine, ops
        self.links = []
        self._mp = pytest.MonkeyPatch()

    def __enter__(self):
        if self.engine is None:
            from dl_vqa_amd import engine, ops
            self.engine, self.ops = engine, ops
        eng, ops, mp = self.engine, self.ops, self._mp
        mp.setenv("VQA_STREAMS", "0")          # read per call (Engine._on_side_stream): everything on one stream
        mp.setattr(eng, "_gemm", self._wrap_gemm(eng._gemm))
        mp.setattr(ops, "gemm_tall_bf16", self._wrap_tall(ops.gemm_tall_bf16))
        mp.setattr(ops, "to_bf16", self._wrap_to_bf16(ops.to_bf16))
        mp.setattr(ops, "add2d", self._wrap_add2d(ops.add2d))
        mp.setattr(eng.Engine, "_rows16", staticmethod(self._wrap_rows16(eng.Engine._rows16)))
        mp.setattr(eng.Engine, "_cols16", staticmethod(self._wrap_cols16(eng.Engine._cols16)))
        return self

    def __exit__(self, *exc):
        self._mp.undo()
        return False

    # ---------------------------------------------------------------- products
    def _product(self, run, engine, plan, A, B, C, M, N, K, transA, transB, lda, ldb, ldc, bias1=None, bias2=None, rowgroup=None,
                 rg_div=1, rg_op=0, relu=False, accumulate=False, aux=None, tag=0):
        groups = -(-M // rg_div) if rowgroup is not None else 0
        link = SimpleNamespace(
            kind="product", tag=tag, engine=engine, plan=plan, M=M, N=N, K=K, transA=transA, transB=transB, lda=lda, ldb=ldb,
            ldc=ldc, rg_div=rg_div, rg_op=rg_op, relu=bool(relu), accumulate=bool(accumulate),
            A=_view(A, M, K, lda, transA).clone(), B=_view(B, K, N, ldb, transB).clone(),
            bias1=_clone(bias1), bias2=_clone(bias2),
            rowgroup=None if rowgroup is None else _view(rowgroup, groups, N, rowgroup.stride(0)).clone(),
            C0=_view(C, M, N, ldc).clone() if accumulate else None, c_ptr=C.data_ptr())
        out = run()
        link.C = _view(C, M, N, ldc).clone()
        link.aux = None if aux is None else _view(aux, M, N, ldc).clone()
        self.links.append(link)
        return out

    def _wrap_gemm(self, real):
        def _gemm(A, B, C, M, N, K, x3=False, **kw):
            engine = BF16 if A.dtype == torch.bfloat16 else (X3 if x3 else F32)
            transA, transB = kw.get("transA", False), kw.get("transB", True)
            lda = kw["lda"] if kw.get("lda") is not None else (M if transA else K)       # as ops._gemm resolves them
            ldb = kw["ldb"] if kw.get("ldb") is not None else (K if transB else N)
            ldc = kw["ldc"] if kw.get("ldc") is not None else N
            plan = self.ops.gemm_plan(engine, M, N, K, transA=transA, transB=transB)
            epi = {k: kw[k] for k in ("bias1", "bias2", "rowgroup", "rg_div", "rg_op", "relu", "accumulate", "aux", "tag") if k in kw}
            return self._product(lambda: real(A, B, C, M, N, K, x3=x3, **kw), engine, plan, A, B, C, M, N, K, transA, transB,
                                 lda, ldb, ldc, **epi)
        return _gemm

    def _wrap_tall(self, real):
        def gemm_tall_bf16(A, W, C, M, N, K, **kw):
            plan = self.ops.gemm_tall_bf16_plan(M, N, K)
            return self._product(lambda: real(A, W, C, M, N, K, **kw), TALL, plan, A, W, C, M, N, K, False, True, A.stride(0),
                                 W.stride(0), C.stride(0), **kw)
        return gemm_tall_bf16

    # ---------------------------------------------------------------- casts and copies
    def _cast(self, name, x, out, rows, cols, rows8, cols8):
        self.links.append(SimpleNamespace(kind="cast", name=name, x=x, out=out.detach().reshape(rows8, cols8).clone(), rows=rows,
                                          cols=cols, rows8=rows8, cols8=cols8, out_ptr=out.data_ptr()))

    def _wrap_to_bf16(self, real):
        def to_bf16(x, out=None):
            x0 = x.detach().clone()
            y = real(x, out=out)
            self._cast("to_bf16", x0.reshape(1, -1), y, 1, x0.numel(), 1, x0.numel())
            return y
        return to_bf16

    def _wrap_rows16(self, real):
        def _rows16(x, ld, rows, cols, rows8):
            x0 = _view(x, rows, cols, ld).clone()
            y = real(x, ld, rows, cols, rows8)
            assert tuple(y.shape) == (rows8, cols), (tuple(y.shape), rows8, cols)
            self._cast("_rows16", x0, y, rows, cols, rows8, cols)
            return y
        return _rows16

    def _wrap_cols16(self, real):
        def _cols16(x, rows, cols, cols8):
            x0 = x.detach().reshape(rows, cols).clone()
            y = real(x, rows, cols, cols8)
            assert tuple(y.shape) == (rows, cols8), (tuple(y.shape), rows, cols8)
            self._cast("_cols16", x0, y, rows, cols, rows, cols8)
            return y
        return _cols16

    def _wrap_add2d(self, real):
        def add2d(a, lda, b, ldb, out, ldo, rows, cols):
            if b is not None:                       # a sum: owned by tests/test_streaming_gpu.py
                return real(a, lda, b, ldb, out, ldo, rows, cols)
            a0 = _view(a, rows, cols, lda).clone()
            y = real(a, lda, b, ldb, out, ldo, rows, cols)
            self.links.append(SimpleNamespace(kind="copy", name="add2d", x=a0, out=_view(out, rows, cols, ldo).clone(), rows=rows,
                                              cols=cols, lda=lda, ldo=ldo, a_ptr=a.data_ptr(), out_ptr=out.data_ptr()))
            return y
        return add2d


# -------------------------------------------------------------------------------------------------- references
def product_ref(link):
    """(raw product = aux, result) of a product link in float64, from the operands as recorded; the epilogue in epi_apply's
    order: row group (add or multiply, row // rg_div), bias1, bias2, ReLU, + C's previous contents."""
    prod = link.A.double().cpu() @ link.B.double().cpu()
    v = prod
    if link.rowgroup is not None:
        g = link.rowgroup.double().cpu()[torch.arange(link.M) // link.rg_div]
        v = v * g if link.rg_op else v + g
    if link.bias1 is not None:
        v = v + link.bias1.double().cpu()
    if link.bias2 is not None:
        v = v + link.bias2.double().cpu()
    if link.relu:
        v = torch.clamp_min(v, 0.0)
    if link.accumulate:
        v = v + link.C0.double().cpu()
    return prod, v


def cast_ref(link):
    """what a cast link's output must be: [rows8][cols8] bf16, the round-to-nearest-even (.to(torch.bfloat16) on the CPU) of the
    fp32 input in the first rows x cols, +0 elsewhere"""
    ref = torch.zeros(link.rows8, link.cols8, dtype=torch.bfloat16)
    ref[:link.rows, :link.cols] = link.x.cpu().reshape(link.rows, link.cols).to(torch.bfloat16)
    return ref


def _bits(t):
    return t.cpu().contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _rel(got, ref):
    return float((got.double().cpu() - ref).abs().max()) / max(float(ref.abs().max()), 1e-300)


def _plan_str(link):
    p = link.plan
    if link.engine == TALL:
        return f"BM={p.get('BM')} grid={p.get('grid')} nk={p.get('nk')}"
    form = "wide" if p.get("wide") else f"{p.get('BM')}x{p.get('BN')}"
    return f"{form} splits={p.get('splits')}{' persistent' if p.get('persistent') else ''}"


def judge(link):
    """(what the link is, measured error, bound, failures) of one link.  Error and bound: an fp32 product max|got - ref| / max|ref|
    against tol_sum(K + 3), aux included; a bf16 product the largest |got - ref| / (2^-8 |ref| + T max|ref|) against 1, judged by
    check_bf16; a cast or copy the number of elements that differ (pads: whose bits differ from +0), against 0."""
    fails = []
    if link.kind == "product":
        what = (f"tag {link.tag} {link.engine} {link.M}x{link.N}x{link.K} {'T' if link.transA else 'N'}{'T' if link.transB else 'N'} "
                f"[{_plan_str(link)}]")
        prod, ref = product_ref(link)
        T = tol_sum(link.K + 3)
        if link.C.dtype == torch.bfloat16:
            got = link.C.double().cpu()
            err = float(((got - ref).abs() / (2.0 ** -8 * ref.abs() + T * float(ref.abs().max())).clamp_min(1e-300)).max())
            bound = 1.0
            try:
                check_bf16(what, link.C, ref, T=T)
            except AssertionError as e:
                fails.append(f"{what}: bf16 result: {e}")
        else:
            err, bound = _rel(link.C, ref), T
            if not err <= bound:
                fails.append(f"{what}: max|got - ref| / max|ref| = {err:.3e} > {bound:.3e}")
        if link.aux is not None:
            e_aux = _rel(link.aux, prod)
            if not e_aux <= T:
                fails.append(f"{what}: aux {e_aux:.3e} > {T:.3e}")
            if link.C.dtype != torch.bfloat16:
                err = max(err, e_aux) if e_aux == e_aux else e_aux
            what += f" aux {e_aux:.3e}"
        return what, err, bound, fails
    if link.kind == "cast":
        what = f"cast {link.name} {link.rows}x{link.cols} -> {link.rows8}x{link.cols8}"
        ref = cast_ref(link)
        assert link.out.dtype == torch.bfloat16, link.out.dtype
        body = int((link.out.cpu()[:link.rows, :link.cols] != ref[:link.rows, :link.cols]).sum())      # -0 == +0; NaN differs
        wrong = _bits(link.out) != _bits(ref)
        pad = int(wrong.sum()) - int(wrong[:link.rows, :link.cols].sum())
        if body:
            fails.append(f"{what}: {body} elements are not the round-to-nearest-even of their source")
        if pad:
            fails.append(f"{what}: {pad} pad elements are not +0")
        return what, float(body + pad), 0.0, fails
    what = f"copy {link.name} {link.rows}x{link.cols} ld {link.lda} -> {link.ldo}"
    wrong = int((link.out.cpu() != link.x.cpu()).sum())
    if wrong:
        fails.append(f"{what}: {wrong} elements differ from their source")
    return what, float(wrong), 0.0, fails


def audit(links, check=True, label=""):
    """One [links] line per link: what it is (tag or cast name, engine, M x N x K, plan), measured error, bound; label: the
    caller's name for the step, printed in front.  Returns the failures (strings, one per finding); check: raises
    AssertionError with all of them after the last line."""
    failures = []
    for i, link in enumerate(links):
        what, err, bound, fails = judge(link)
        print(f"[links] {label}{i:3d} {what}: error {err:.3e} bound {bound:.3e} {'FAIL' if fails else 'ok'}")
        failures += fails
    if check and failures:
        raise AssertionError(f"{len(failures)} link finding(s):\n  " + "\n  ".join(failures))
    return failures


def products(links, *tags):
    return [l for l in links if l.kind == "product" and (not tags or l.tag in tags)]


def casts(links, name=None):
    return [l for l in links if l.kind == "cast" and (name is None or l.name == name)]


def narrowing(links, product):
    """the copy link that read the result of `product` (by address), or None"""
    after = links[[id(l) for l in links].index(id(product)) + 1:]
    return next((l for l in after if l.kind == "copy" and l.a_ptr == product.c_ptr), None)
