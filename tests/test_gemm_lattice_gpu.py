"""vqa_gemm, vqa_gemm_x3, vqa_gemm_bf16 and vqa_gemm_tall_bf16 bit for bit, in every plan the train step runs, on operands whose
arithmetic is exact.

tests/gemm_lattice_ref.py draws the operands from a dyadic lattice of bf16 values on which every partial sum, split-K slab and
epilogue step is an fp32 value, so each fp32 output must EQUAL the float64 closed form and each bf16 output its
round-to-nearest-even, whatever the tile, launch form, split count or reduce kernel.  tests/test_gemm_lattice_ref_cpu.py holds
the reference to float64 matmul and shows which kernel every case below runs; here each case asserts the plan it is listed
for through ops.gemm_plan before it calls the entry point.

Every operand is a view into a NaN-filled buffer (NaN between the row length and the leading dimension, in the rows after
the last one, before and after the matrix), C and aux are NaN-filled too and the split-K workspace is filled with NaN before
each call: an unmasked operand element or an unwritten output element cannot compare equal, and everything outside
C[M][N] / aux[M][N] must keep its NaN bit for bit.  One `[lattice]` line per case: the case, its plan, elements compared,
mismatches (asserted to be 0).
"""
import os

import pytest
import torch

from tests import gemm_lattice_ref as L

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
BF16, F32 = torch.bfloat16, torch.float32


class _PoisoningTorch:
    """`torch` as dl_vqa_amd.ops sees it during these tests: empty() returns NaN instead of whatever was there."""

    def __getattr__(self, name):
        return getattr(torch, name)

    @staticmethod
    def empty(*size, dtype=F32, device=None):
        return torch.empty(*size, dtype=dtype, device=device).fill_(NAN)


@pytest.fixture(autouse=True)
def ops(monkeypatch):
    from dl_vqa_amd import ops as _ops
    monkeypatch.setattr(_ops, "torch", _PoisoningTorch())
    monkeypatch.setattr(_ops, "_ws", {})                       # a fresh, poisoned workspace
    assert bool(torch.isnan(_ops.workspace(64, torch.device(DEV))).all())
    return _ops


@pytest.fixture
def knobs(monkeypatch):
    """The library under exactly the VQA_* knobs a case lists (it reads them once: vqa_reload_knobs after every change and
    after the test's environment has been restored)."""
    from dl_vqa_amd import _lib

    def set_knobs(pairs):
        for k in [k for k in os.environ if k.startswith("VQA_") and k != "VQA_LIB"]:
            monkeypatch.delenv(k)
        for name, value in pairs:
            monkeypatch.setenv(name, value)
        _lib.load().vqa_reload_knobs()
    yield set_knobs
    monkeypatch.undo()
    _lib.load().vqa_reload_knobs()


class Tally:
    """Exact comparisons of one case; prints the case's [lattice] line and fails after it if anything differed."""

    def __init__(self, c, plan, plan_text=None):
        self.c, self.plan, self.n, self.bad, self.where, self.plan_text = c, plan, 0, 0, [], plan_text

    def eq(self, name, got, want):
        """got == want element for element (-0 equals +0, NaN equals nothing); a float64 reference is narrowed to got's type"""
        got = got.detach().cpu()
        if want.dtype == torch.float64:
            want = L.rne_bf16(want) if got.dtype == BF16 else want.to(F32)
        assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, want.shape, got.dtype, want.dtype)
        self.n += got.numel()
        if not torch.equal(got, want):
            ne = got != want
            self.bad += int(ne.sum())
            first = [int(v) for v in ne.nonzero()[0]]
            self.where.append(f"{name}: {int(ne.sum())} of {got.numel()} differ, first at {first}: "
                              f"got {got[tuple(first)].item()} want {want[tuple(first)].item()}")

    def untouched(self, name, after, before):
        """integer views of everything outside a matrix: the NaN fill, bit for bit"""
        self.n += after.numel()
        if not torch.equal(after.cpu(), before):
            ne = after.cpu() != before
            self.bad += int(ne.sum())
            self.where.append(f"{name}: {int(ne.sum())} elements outside the matrix were written")

    def done(self):
        p = self.plan
        text = self.plan_text or (f"{p['BM']}x{p['BN']} tiles {p['tiles_m']}x{p['tiles_n']} nk {p['nk']} splits {p['splits']}x"
                                  f"{p['ks_per_split']} order {p['order']} persistent {p['persistent']} wide {p['wide']}")
        print(f"[lattice] {L.case_id(self.c)}: {text}; compared {self.n} mismatches {self.bad}")
        assert self.bad == 0 and not self.where, "\n".join(self.where)


def run(ops, set_knobs, c, expect_plan=True):
    """one case: its knobs, its plan (asserted), poisoned operands, the call, the exact comparison; returns the plan"""
    from dl_vqa_amd import _lib
    set_knobs(c.knobs)
    M, N, K, e = c.M, c.N, c.K, c.epi
    dt = BF16 if c.engine == L.BF16 else F32
    nbytes = getattr(_lib.load(), c.engine + "_workspace_bytes")(M, N, K)
    ws = ops.workspace(nbytes, torch.device(DEV)).fill_(NAN) if nbytes else None
    plan = ops.gemm_plan(c.engine, M, N, K, transA=c.transA, transB=c.transB, workspace_bytes=ws.numel() * 4 if nbytes else 0)
    if expect_plan:
        assert {k: plan[k] for k in c.plan} == c.plan, (L.case_id(c), c.plan, plan)
    A, B = L.operands(c.lattice, M, N, K)
    b1, b2, rg, c0 = L.extras(c)
    prod, want = L.expected(c)
    lda, ldb, ldc, rg_ld = L.leading_dims(c)
    a_rows, a_cols = (K, M) if c.transA else (M, K)
    b_rows, b_cols = (N, K) if c.transB else (K, N)
    Ad = L.stored((A.t() if c.transA else A).contiguous(), a_rows, a_cols, lda, dt).to(DEV)
    Bd = L.stored((B.t() if c.transB else B).contiguous(), b_rows, b_cols, ldb, dt).to(DEV)
    vec = lambda v: None if v is None else L.stored(v.view(1, N), 1, N, N + 3, F32).to(DEV)[L.LEAD:]
    rgd = None if rg is None else L.body(L.stored(rg, rg.shape[0], N, rg_ld, F32).to(DEV), rg.shape[0], N, rg_ld)
    assert rgd is None or (rgd.stride(0) == rg_ld > N and rgd.data_ptr() % 16 == 0)
    lead_c = L.LEAD + c.c_off
    C_cpu = L.stored(c0, M, N, ldc, BF16 if c.c_bf16 else F32, lead=lead_c)
    aux_cpu = L.stored(None, M, N, ldc, F32) if e.aux else None
    Cd, auxd = C_cpu.to(DEV), (aux_cpu.to(DEV) if e.aux else None)
    assert Ad.data_ptr() % 16 == 0 and Bd.data_ptr() % 16 == 0 and (Cd[lead_c:].data_ptr() % 16 == 0) == (c.c_off % 8 == 0)
    kw = dict(transA=c.transA, transB=c.transB, lda=lda, ldb=ldb, ldc=ldc, bias1=vec(b1), bias2=vec(b2), rowgroup=rgd,
              rg_div=e.rg_div or 1, rg_op=e.rg_op, relu=e.relu, accumulate=e.accumulate, aux=None if auxd is None else auxd[L.LEAD:])
    if c.engine == L.BF16:
        ops.gemm_bf16(Ad[L.LEAD:], Bd[L.LEAD:], Cd[lead_c:], M, N, K, **kw)
    else:
        ops.gemm(Ad[L.LEAD:], Bd[L.LEAD:], Cd[lead_c:], M, N, K, x3=c.engine == L.X3, **kw)
    torch.cuda.synchronize()
    t = Tally(c, plan)
    t.eq("C", L.body(Cd, M, N, ldc, lead_c), want)
    t.untouched("C", L.outside(Cd, M, N, ldc, lead_c), L.outside(C_cpu, M, N, ldc, lead_c))
    if e.aux:
        t.eq("aux", L.body(auxd, M, N, ldc), prod)
        t.untouched("aux", L.outside(auxd, M, N, ldc), L.outside(aux_cpu, M, N, ldc))
    t.done()
    return plan


def ids(cases):
    return [L.case_id(c) for c in cases]


# ----------------------------------------------------------------------------- tile geometry x K tails x layouts
@pytest.mark.parametrize("engine", [L.F32, L.BF16])
@pytest.mark.parametrize("rows", [130, 256, 300])
def test_tile_geometry(ops, knobs, engine, rows):
    """128 x 128 and 256 x 128 tiles, plain and persistent, at the smallest shapes that have them (VQA_SPLIT_TARGET=1): all-edge
    (130 x 130), all-interior (256 x 384) and mixed (300 x 260) tilings; K with a straddling chunk, an exact multiple, a
    whole-chunk tail and a one-element tail; every layout.  PlainC's unmasked columns beyond `cols` read NaN here."""
    cases = [c for c in L.cases_of("geometry") if c.engine == engine and L.roundup(c.M, 8) == L.roundup(rows, 8)]
    assert len(cases) == (68 if engine == L.F32 else 16)
    for c in cases:
        run(ops, knobs, c)


# ----------------------------------------------------------------------------- the planner's own choices
@pytest.mark.parametrize("c", L.cases_of("real"), ids=ids(L.cases_of("real")))
def test_planner_choices(ops, knobs, c):
    """210 tiles of 128 x 128 persistent (short K), plain (long K) and with two splits; the skinny shape in tile order 1, split
    as the planner has it and unsplit on both kernels."""
    run(ops, knobs, c)


@pytest.mark.parametrize("c", L.cases_of("walk"), ids=ids(L.cases_of("walk")))
def test_persistent_workgroups_walk_several_tiles(ops, knobs, c):
    """More tiles than the persistent grid has workgroups (at most two per CU, one for 256 x 128 tiles), so workgroups
    re-initialise their loaders at a tile seam and the last round is partial; the plain kernel must give the same bits."""
    slots = (2 if c.plan["BM"] == 128 else 1) * torch.cuda.get_device_properties(0).multi_processor_count
    tiles = c.plan["tiles_m"] * c.plan["tiles_n"]
    assert tiles > slots and tiles % slots != 0, (tiles, slots)
    run(ops, knobs, c)


# ----------------------------------------------------------------------------- the fused epilogue
@pytest.mark.parametrize("engine,bm", [(L.F32, 64), (L.F32, 128), (L.F32, 256), (L.BF16, 64), (L.BF16, 128)])
def test_epilogue_matrix(ops, knobs, engine, bm):
    """every gemm_epilogue_mode instantiation of a tile size: row groups below, at and above the tile height and with a partial
    last tile, add / multiply, biases, ReLU, accumulate, aux, fp32 and bf16 C"""
    cases = [c for c in L.cases_of("epilogue") if c.engine == engine and c.plan["BM"] == bm]
    assert len(cases) >= 24
    for c in cases:
        run(ops, knobs, c)


@pytest.mark.parametrize("c", L.cases_of("staged"), ids=ids(L.cases_of("staged")))
def test_bf16_staged_epilogue(ops, knobs, c):
    """gemm_epilogue_bf16_staged on interior tiles, the direct stores on edge tiles of the same launch and wherever ldc or C's
    alignment rule the staged form out: the same bits"""
    plan = run(ops, knobs, c)
    assert L.runs_staged(c, plan) == (L.leading_dims(c)[2] % 8 == 0 and c.c_off == 0)


# ----------------------------------------------------------------------------- split-K and its reduce kernels
@pytest.mark.parametrize("engine", [L.F32, L.BF16])
def test_split_counts(ops, knobs, engine):
    """2 to 52 splits through both reduce kernels: thread groups of splitk_reduce4_kernel left empty (2, 3 splits), its odd tail
    (5, 9, 13), a last split of one one-element K-step; the epilogue applied by the reduce kernel"""
    cases = [c for c in L.cases_of("split") if c.engine == engine]
    assert {c.plan["splits"] for c in cases} >= ({2, 3, 4, 5, 9, 13, 14, 52} if engine == L.F32 else {3, 5, 9, 13})
    for c in cases:
        run(ops, knobs, c)


@pytest.mark.parametrize("c", L.cases_of("wide"), ids=ids(L.cases_of("wide")))
def test_bf16_long_k_weight_gradient(ops, knobs, c):
    """128 x 256 tiles where the ordinary plan's workspace holds the wide plan's slabs (128 rows, a fresh workspace), the
    ordinary plan where it does not (256 rows): whichever the query reports for the workspace this call passes"""
    plan = run(ops, knobs, c)
    ws_bytes = ops.workspace(0, torch.device(DEV)).numel() * 4
    assert plan["wide"] == int(ws_bytes >= 64 * c.M * c.N * 4) == int(c.M == 128), (plan, ws_bytes)
    assert (plan["BM"], plan["BN"]) == ((128, 256) if plan["wide"] else (64, 64))


# ----------------------------------------------------------------------------- 3 x bf16
def test_x3_tiles_epilogue_and_plane_lattices(ops, knobs):
    """vqa_gemm_x3's 192 x 128 tiles in one launch and split along K, its epilogue, and the three plane lattices that reach the
    hm / mh / mm and hl / lh products (tests/test_x3_gpu.py stays the judge of the split arithmetic on ordinary data)"""
    cases = L.cases_of("x3")
    assert len(cases) == 25
    for c in cases:
        run(ops, knobs, c)


@pytest.mark.parametrize("c", L.cases_of("x3walk"), ids=ids(L.cases_of("x3walk")))
def test_x3_persistent_workgroups_walk_several_tiles(ops, knobs, c):
    """272 tiles on the persistent kernel's 256 workgroups (16 of them take a second tile), and one tile per workgroup"""
    assert c.plan["tiles_m"] * c.plan["tiles_n"] == 272
    run(ops, knobs, c)


# ----------------------------------------------------------------------------- the tall bf16 engine
@pytest.mark.parametrize("c", L.tall_cases_both_heights(), ids=ids(L.tall_cases_both_heights()))
def test_tall_bf16(ops, knobs, c):
    """vqa_gemm_tall_bf16, every case on 256-row and (VQA_TALL_BM=128) on 128-row tiles: one tile per workgroup with one, two and three
    k-stages, tile seams with the row-group table's minimum lead, tiles that span two row groups, a partial last group, a last
    row tile partly past M, three tiles per workgroup, a grid that is no multiple of 8, with and without ReLU.  Every bf16
    output equals the round-to-nearest-even of the float64 result; the pad columns of C and the guard rows after row M - 1
    keep their NaN bits."""
    knobs(c.knobs)
    M, N, K, e = c.M, c.N, c.K, c.epi
    assert ops.gemm_tall_bf16_supported(M, N, K, e.rg_div, bool(e.rg_div))
    plan = ops.gemm_tall_bf16_plan(M, N, K)
    assert {k: plan[k] for k in c.plan} == c.plan, (L.case_id(c), c.plan, plan)
    A, B = L.operands(c.lattice, M, N, K)
    rg = L.extras(c)[2]
    want = L.expected(c)[1]
    lda, ldw, ldc, rg_ld = L.leading_dims(c)
    Ad = L.stored(A, M, K, lda, BF16).to(DEV)
    Wd = L.stored(B.t().contiguous(), N, K, ldw, BF16).to(DEV)
    rgd = None if rg is None else L.body(L.stored(rg, rg.shape[0], N, rg_ld, F32).to(DEV), rg.shape[0], N, rg_ld)
    assert rgd is None or (rgd.shape[0] == -(-M // e.rg_div) and rgd.stride(0) == rg_ld > N and rgd.data_ptr() % 16 == 0)
    C_cpu = L.stored(None, M, N, ldc, BF16)
    Cd = C_cpu.to(DEV)
    a, w, cv = L.body(Ad, M, K, lda), L.body(Wd, N, K, ldw), L.body(Cd, M, N, ldc)
    assert a.stride(0) == lda and w.stride(0) == ldw and cv.stride(0) == ldc
    assert a.data_ptr() % 16 == 0 and w.data_ptr() % 16 == 0 and cv.data_ptr() % 16 == 0
    ops.gemm_tall_bf16(a, w, cv, M, N, K, rowgroup=rgd, rg_div=e.rg_div or 1, rg_op=e.rg_op, relu=e.relu)
    torch.cuda.synchronize()
    t = Tally(c, plan, f"{plan['BM']}-row tiles {plan['tiles_m']}x{plan['tiles_n']} grid {plan['grid']} nk {plan['nk']}")
    t.eq("C", L.body(Cd, M, N, ldc), want)
    t.untouched("C", L.outside(Cd, M, N, ldc), L.outside(C_cpu, M, N, ldc))
    t.done()
