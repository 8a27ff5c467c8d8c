"""CPU: the reference of tests/gemm_lattice_ref.py, the exactness of every case of tests/test_gemm_lattice_gpu.py, and what that
case table COVERS -- ops.gemm_plan (vqa_gemm_plan: the planners and persistent rules the launchers use, no HIP call) says which
kernel each case runs, here, without a GPU."""
import os

import pytest
import torch

from tests import gemm_lattice_ref as L


@pytest.fixture
def knob(monkeypatch):
    """the library with exactly the VQA_* knobs a case lists (read once: vqa_reload_knobs after every change and after the test)"""
    from dl_vqa_amd import _lib
    lib = _lib.load()

    def set_knobs(knobs):
        for k in [k for k in os.environ if k.startswith("VQA_") and k != "VQA_LIB"]:
            monkeypatch.delenv(k)
        for name, value in knobs:
            monkeypatch.setenv(name, value)
        lib.vqa_reload_knobs()
    yield set_knobs
    monkeypatch.undo()
    lib.vqa_reload_knobs()


def plan_of(c):
    from dl_vqa_amd import ops
    return ops.gemm_plan(c.engine, c.M, c.N, c.K, transA=c.transA, transB=c.transB)


SMALL = [c for c in L.all_cases() if c.M * c.N * c.K <= 1 << 26]


def test_reference_is_float64_matmul_plus_spelled_out_epilogue():
    seen = set()
    for c in SMALL:
        if (c.epi, c.lattice) in seen:
            continue
        seen.add((c.epi, c.lattice))
        A, B = L.operands(c.lattice, c.M, c.N, c.K)
        b1, b2, rg, c0 = L.extras(c)
        prod, want = L.expected(c)
        raw = torch.matmul(A.double(), B.double())
        assert raw.dtype == torch.float64 and torch.equal(prod, raw)
        e = c.epi
        v = raw.clone()
        for row in range(c.M):                                # epi_apply, one row at a time
            if e.rg_div:
                g = rg[row // e.rg_div]
                v[row] = v[row] * g if e.rg_op else v[row] + g
            if e.nbias >= 1:
                v[row] += b1
            if e.nbias == 2:
                v[row] += b2
            if e.relu:
                v[row] = torch.where(v[row] > 0, v[row], torch.zeros(()).double())
            if e.accumulate:
                v[row] += c0[row]
        assert torch.equal(v, want), L.case_id(c)
        if e.rg_div:
            assert rg.shape[0] * e.rg_div == c.M and (e.rg_op == 0 or bool((rg != 0).all()))
    assert len(seen) > 60


def test_every_case_meets_the_exactness_condition():
    worst = {}
    for c in L.all_cases():
        bound = L.assert_exact(c)
        key = "plane lattices" if c.lattice.startswith("x3") else "bf16-exact lattice"
        worst[key] = max(worst.get(key, 0.0), bound)
    print(f"[lattice] {len(L.all_cases())} cases; largest bound {worst} (limits {L.LIMIT}, {L.LIMIT_X3})")
    assert max(c.K for c in L.all_cases()) == 65536
    # the condition can fail: a longer K than a plane lattice carries, an epilogue on one, an operand off the lattice
    with pytest.raises(AssertionError):
        L.assert_exact(L.Case("x", L.X3, 200, 130, 400, lattice="x3iii"))
    with pytest.raises(AssertionError):
        L.assert_exact(L.Case("x", L.X3, 200, 130, 16, epi=L.Epi(nbias=1), lattice="x3i"))
    with pytest.raises(AssertionError):
        L.assert_exact(L.Case("x", L.X3, 200, 130, 200, lattice="x3i"))


def test_operand_lattice():
    A, B = L.operands("std", 300, 260, 512)
    assert float(A.abs().max()) == 4 and L.on_lattice(A, 1.0) and float(B.abs().max()) == 2 and L.on_lattice(B, 0.5)
    assert 0.30 < float((B == 0).double().mean()) < 0.37
    assert not L.on_lattice(B, 1.0) and len(A.unique()) == 9 and len(B.unique()) == 9


def test_bf16_expectation_rounds_to_nearest_even_with_ties():
    t = torch.tensor([1.0 + 2 ** -8, 1.0 + 3 * 2 ** -8, 257.0, 259.0, 258.0, -0.0, 1.0 + 2 ** -9]).double()
    assert torch.equal(L.rne_bf16(t), t.to(torch.bfloat16))
    assert L.rne_bf16(t).tolist() == [1.0, 1.0 + 2 ** -6, 256.0, 260.0, 258.0, 0.0, 1.0]
    assert L.bf16_stats(t) == (5 / 7, 4)
    with pytest.raises(AssertionError):
        L.rne_bf16(torch.tensor([1.0 + 2 ** -30], dtype=torch.float64))
    n = 0
    for c in L.all_cases():
        if c.c_bf16 and c.M * c.N * c.K <= 1 << 29:
            want = L.expected(c)[1]
            assert torch.equal(L.rne_bf16(want), want.to(torch.bfloat16))
            unrep, ties = L.bf16_stats(want)
            n += 1
            if n % 8 == 1:
                print(f"[lattice] {L.case_id(c)}: {100 * unrep:.1f} % of the outputs are no bf16 values, {ties} exact ties")
            assert unrep >= 0.05 and ties >= 20, (L.case_id(c), unrep, ties)
    assert n >= 30 and any(c.lattice == "std16" for c in L.all_cases() if c.c_bf16)


def test_x3_plane_lattices_split_as_the_kernel_splits():
    """vqa_x3_split's rule (hi = RNE(x), mid = RNE(x - hi), lo = the rest) on the plane lattices: (i) / (ii) fill all three planes
    with exactly their digits, (iii) fills hi and mid; the issue's 65536 h + 256 m + l would leave lo empty."""
    A, B = L.operands("x3i", 200, 130, 16)
    hi, mid, lo = L.x3_planes(A)
    assert set(hi.unique().tolist()) == {-3 * 2.0 ** 17, 3 * 2.0 ** 17} and set(mid.unique().tolist()) == {-768.0, 768.0}
    assert set(lo.unique().tolist()) == {-1.0, 0.0, 1.0} and float((lo != 0).double().mean()) > 0.6
    assert torch.equal(hi + mid + lo, A) and all(float(p.abs().max()) == 0 for p in L.x3_planes(B)[1:])
    A2, B2 = L.operands("x3ii", 200, 130, 16)
    assert float((L.x3_planes(B2)[2] != 0).double().mean()) > 0.6 and all(float(p.abs().max()) == 0 for p in L.x3_planes(A2)[1:])
    for t in L.operands("x3iii", 200, 130, 200):
        hi, mid, lo = L.x3_planes(t)
        assert float(lo.abs().max()) == 0 and float((mid != 0).double().mean()) > 0.15 and torch.equal(hi + mid, t)
    g = torch.Generator().manual_seed(0)
    naive = 65536 * L._digits(g, (4096,)) + 256 * L._digits(g, (4096,)) + L._digits(g, (4096,))
    assert float(L.x3_planes(naive)[2].abs().max()) == 0
    assert [float(p) for p in L.x3_planes(torch.tensor([65793.0]).double())] == [66048.0, -255.0, 0.0]


def test_poisoned_storage():
    m = torch.arange(12.0).double().view(3, 4)
    for dtype, ints in ((torch.float32, torch.int32), (torch.bfloat16, torch.int16)):
        flat = L.stored(m, 3, 4, 7, dtype)
        assert flat.numel() == L.LEAD + (3 + L.GUARD_ROWS) * 7 + L.TAIL and L.LEAD * flat.element_size() % 16 == 0
        assert torch.equal(L.body(flat, 3, 4, 7).double(), m)
        out = L.outside(flat, 3, 4, 7)
        assert out.numel() == flat.numel() - 12 and out.dtype == ints and len(out.unique()) == 1
        assert bool(torch.isnan(flat[:L.LEAD]).all()) and bool(torch.isnan(flat[L.LEAD + 4:L.LEAD + 7]).all())
        assert bool(torch.isnan(flat[L.LEAD + 3 * 7:]).all())
    with pytest.raises(AssertionError):
        L.stored(torch.tensor([[1.0 + 2 ** -12]]).double(), 1, 1, 4, torch.bfloat16)


def test_plan_query_needs_no_gpu(knob):
    from dl_vqa_amd import _lib, ops
    knob(())
    p = ops.gemm_plan(L.F32, 1700, 1850, 72)
    assert p == dict(BM=128, BN=128, tiles_m=14, tiles_n=15, nk=3, splits=1, ks_per_split=3, order=0, persistent=1, wide=0)
    knob((("VQA_PERSISTENT", "0"),))
    assert ops.gemm_plan(L.F32, 1700, 1850, 72)["persistent"] == 0
    knob(())
    assert ops.gemm_plan(L.F32, 64, 64, 32)["persistent"] == 0          # never below 128-row tiles
    assert ops.gemm_plan(L.X3, 3254, 2042, 40)["persistent"] == 1 and ops.gemm_plan(L.X3, 3072, 2048, 40)["persistent"] == 0
    wide = dict(transA=True, transB=False)
    assert ops.gemm_plan(L.BF16, 128, 256, 65536, **wide)["wide"] == 1 and ops.gemm_plan(L.BF16, 128, 256, 65536)["wide"] == 0
    assert ops.gemm_plan(L.BF16, 128, 256, 65536, workspace_bytes=0, **wide)["wide"] == 0
    assert ops.gemm_plan(L.BF16, 256, 256, 65536, workspace_bytes=1 << 24, **wide) == dict(
        BM=128, BN=256, tiles_m=2, tiles_n=1, nk=1024, splits=64, ks_per_split=16, order=0, persistent=0, wide=1)
    for name in (L.F32, L.X3, L.BF16):                               # the plan's slabs are what *_workspace_bytes reports
        for M, N, K in ((256, 1024, 2560), (64, 64, 256), (1700, 1850, 2100)):
            p = ops.gemm_plan(name, M, N, K, workspace_bytes=0)
            assert getattr(_lib.load(), name + "_workspace_bytes")(M, N, K) == (p["splits"] * M * N * 4 if p["splits"] > 1 else 0)
    with pytest.raises(_lib.VqaHipError, match="vqa_gemm_plan: bad args"):
        ops.gemm_plan(L.F32, 0, 64, 64)


def test_every_case_runs_the_plan_it_is_listed_for(knob):
    for c in L.all_cases():
        knob(c.knobs)
        p = plan_of(c)
        assert c.plan is not None and {k: p[k] for k in c.plan} == c.plan, (L.case_id(c), c.plan, p)


def test_the_table_covers_every_kernel_of_the_three_engines(knob):
    """Engine x tile x launch form x layout, the seven gemm_epilogue_mode instantiations on every fp32 and bf16 tile, the staged
    and the direct bf16 epilogue, both reduce kernels and both tile orders: every cell is filled by a case of the GPU table.
    Cells that do not exist: 64 x 64 tiles have no persistent kernel, a split plan never takes 256 x 128 tiles, the wide plan
    always splits and has one layout."""
    cells = {}
    for c in L.all_cases():
        knob(c.knobs)
        p = plan_of(c)
        eng, tile, form = c.engine, L.tile_name(p), L.launch_form(p)
        layout = "TN"[not c.transA] + "TN"[not c.transB]
        found = [("kernel", eng, tile, form, layout), ("order", eng, p["order"])]
        if eng != L.X3:
            if form != "split-K":
                found.append(("epilogue instantiation", eng, tile) + L.epilogue_instantiation(c, p["BM"]))
            found.append(("bf16 epilogue", "staged" if L.runs_staged(c, p) else "direct") if c.c_bf16 and eng == L.BF16 else None)
        if form == "split-K":
            found.append(("reduce kernel", "vector" if c.N % 4 == 0 else "scalar", eng))
        for cell in found:
            if cell is not None:
                cells.setdefault(cell, L.case_id(c))
    layouts = ("NT", "NN", "TT", "TN")
    want = [("kernel", L.F32, t, f, l) for t, forms in (("64x64", ("plain", "split-K")), ("128x128", ("plain", "persistent", "split-K")),
                                                      ("256x128", ("plain", "persistent"))) for f in forms for l in layouts]
    want += [("kernel", L.BF16, t, f, l) for t in ("64x64", "128x128") for f in ("plain", "split-K") for l in layouts]
    want += [("kernel", L.BF16, "wide", "split-K", "TN")]
    want += [("kernel", L.X3, "192x128", f, l) for f in ("plain", "persistent", "split-K") for l in layouts]
    inst = [(0, False, False), (0, True, False), (1, False, False), (0, False, True), (1, True, True), (2, True, True), (0, True, True)]
    want += [("epilogue instantiation", e, t) + i for e, tiles in ((L.F32, ("64x64", "128x128", "256x128")), (L.BF16, ("64x64", "128x128")))
             for t in tiles for i in inst]
    want += [("bf16 epilogue", "staged"), ("bf16 epilogue", "direct")]
    want += [("reduce kernel", k, e) for k in ("vector", "scalar") for e in (L.F32, L.X3, L.BF16)]
    want += [("order", L.F32, 0), ("order", L.F32, 1), ("order", L.BF16, 0), ("order", L.BF16, 1)]
    for cell in want:
        print(f"[coverage] {cell}: {cells.get(cell, 'NOT COVERED')}")
    missing = [cell for cell in want if cell not in cells]
    assert not missing, missing
    assert len(want) == 28 + 17 + 12 + 35 + 2 + 6 + 4
