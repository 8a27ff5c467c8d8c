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


# ----------------------------------------------------------------------------- the tall bf16 engine
def tall_plan(c):
    from dl_vqa_amd import ops
    return ops.gemm_tall_bf16_plan(c.M, c.N, c.K)


def test_tall_cases_are_exact_and_exercise_the_bf16_rounding():
    """With K <= 512, sum |a| |b| max|rg| <= 2^15 (2^15 + 2 at K = 1024, added): far below 2^21, so the float64 result is the only
    correct fp32 value and its round-to-nearest-even the only correct bf16 output -- and that rounding is at work: at least 3 % of
    the expected values are no bf16 values and at least 1000 are exact ties, in every case."""
    ids = [L.case_id(c) for c in L.tall_cases()]
    assert len(set(ids)) == len(ids) == 16
    for c in L.tall_cases():
        assert c.lattice == "std16" and c.c_bf16 and L.assert_exact(c) <= 2.0 ** 15 + 2
        A, B = L.operands(c.lattice, c.M, c.N, c.K)
        assert float(A.abs().max()) == 16 and float(B.abs().max()) == 2 and L.on_lattice(B, 0.5)
        want = L.expected(c)[1]
        assert torch.equal(L.rne_bf16(want), want.to(torch.bfloat16))
        unrep, ties = L.bf16_stats(want)
        print(f"[lattice] {L.case_id(c)}: {100 * unrep:.1f} % of the outputs are no bf16 values, {ties} exact ties")
        assert unrep >= 0.03 and ties >= 1000, (L.case_id(c), unrep, ties)
        assert bool((want < 0).any()) == (not c.epi.relu)             # without ReLU negative outputs must survive
        lda, ldw, ldc, rg_ld = L.leading_dims(c)
        assert (lda, ldw, ldc, rg_ld) == (c.K + 8, c.K + 16, c.N + 8, c.N + 8)


def test_tall_partial_last_row_group():
    c = next(c for c in L.tall_cases() if c.why == "partial-group")
    rg = L.extras(c)[2]
    assert c.M % c.epi.rg_div == 508 and rg.shape == (17, c.N)
    want = L.expected(c)[1]
    prod = L.product(c.lattice, c.M, c.N, c.K)
    assert torch.equal(want[16 * 512:], torch.clamp_min(prod[16 * 512:] + rg[16], 0.0))


def test_tall_plan_query_and_its_knob(knob):
    """vqa_gemm_tall_bf16_plan is what the launcher calls; VQA_TALL_BM is a knob like the others: re-read by vqa_reload_knobs,
    and anything but 128 keeps the 256-row tiles."""
    from dl_vqa_amd import _lib, ops
    knob(())
    assert ops.gemm_tall_bf16_plan(8788, 1024, 256) == dict(BM=256, tiles_m=35, tiles_n=8, grid=256, nk=4)
    knob(L.TALL128)
    assert ops.gemm_tall_bf16_plan(8788, 1024, 256) == dict(BM=128, tiles_m=69, tiles_n=8, grid=512, nk=4)
    for other in ("256", "64", "0", "", "x"):
        knob((("VQA_TALL_BM", other),))
        assert ops.gemm_tall_bf16_plan(8788, 1024, 256)["BM"] == 256, other
    knob(())
    assert ops.gemm_tall_bf16_plan(2048, 1024, 64)["grid"] == 64
    for bad in ((0, 128, 64), (256, 100, 64), (256, 128, 96)):
        with pytest.raises(_lib.VqaHipError, match="vqa_gemm_tall_bf16_plan: bad args"):
            ops.gemm_tall_bf16_plan(*bad)


def _tiles_spanning_two_groups(c, p):
    return sum(1 for mt in range(p["tiles_m"])
               if mt * p["BM"] // c.epi.rg_div != (min((mt + 1) * p["BM"], c.M) - 1) // c.epi.rg_div)


def test_every_tall_case_reaches_the_mechanism_it_is_listed_for(knob):
    """From the launch geometry the launcher itself uses: tiles against grid, tiles per workgroup, the XCD swizzle's remainder,
    the k-stage count against the row-group table's lead, and where the group boundaries fall in the tiles."""
    from dl_vqa_amd import ops
    seen = set()
    for c in L.tall_cases():
        knob(c.knobs)
        p = tall_plan(c)
        assert {k: p[k] for k in c.plan} == c.plan, (L.case_id(c), c.plan, p)
        e = c.epi
        assert ops.gemm_tall_bf16_supported(c.M, c.N, c.K, e.rg_div, bool(e.rg_div)), L.case_id(c)
        bm, tiles, grid, nk = p["BM"], p["tiles_m"] * p["tiles_n"], p["grid"], p["nk"]
        per_wg = -(-tiles // grid)
        assert grid == min(tiles, 65536 // bm) and (not e.rg_div or (e.rg_div >= 256 and nk >= 3))
        if c.why == "nk1":           # the prologue's second load is already the next tile, or past the end
            assert nk == 1 and tiles == grid and not e.rg_div
        elif c.why == "nk2":
            assert nk == 2 and tiles == grid and not e.rg_div
        elif c.why == "group-per-tile":      # the smallest nk with a table; every boundary on a tile seam
            assert nk == 3 and tiles == grid and e.rg_div == bm and _tiles_spanning_two_groups(c, p) == 0
        elif c.why == "one-group":
            assert nk == 3 and tiles == grid and e.rg_div == c.M and e.rg_op == 1
        elif c.why == "seam":        # a second tile whose table load falls in its first stage; a last row tile partly past M
            assert nk == 3 and tiles > grid and per_wg == 2 and tiles % grid == (16 if bm == 256 else 32) and e.rg_op == 1
            assert _tiles_spanning_two_groups(c, p) > (p["tiles_m"] // 2 if bm == 256 else p["tiles_m"] // 3)
            assert 0 < p["tiles_m"] * bm - c.M < bm
        elif c.why == "train":
            assert (c.M, e.rg_div, nk, tiles, grid) == (13 * 676, 676, 4, 280, 256) and per_wg == 2 and 0 < p["tiles_m"] * bm - c.M < bm
        elif c.why == "three-tiles":
            assert tiles == 513 and grid == 256 and per_wg == 3 and tiles % grid == 1 and p["tiles_n"] & (p["tiles_n"] - 1)
            assert c.M == 15 * e.rg_div and e.rg_op == 1 and nk == 8
        elif c.why == "odd-grid":    # xcd_swizzle with a remainder; one column tile
            assert p["tiles_n"] == 1 and tiles == grid and grid % 8 != 0 and nk in (1, 3) and (nk == 1) == (e.rg_div == 0)
        elif c.why == "partial-group":
            assert c.M % e.rg_div != 0 and tiles > grid and nk == 4
        elif c.why == "long-k":
            assert nk == 16 and tiles == grid and e.rg_div == 1024
        else:
            raise AssertionError(c.why)
        seen.add((c.why, bm))
    assert {w for w, bm in seen if bm == 256} == {"nk1", "nk2", "group-per-tile", "one-group", "seam", "train", "three-tiles",
                                                  "odd-grid", "partial-group", "long-k"}
    assert {w for w, bm in seen if bm == 128} == {"seam", "odd-grid", "nk1"}
    assert {c.epi.relu for c in L.tall_cases() if c.why == "train"} == {False, True}
    # the GPU file runs every case under both tile heights; the restated 128-row geometry is the query's
    both = L.tall_cases_both_heights()
    assert len(both) == 26 and len({L.case_id(c) for c in both}) == 26 and sum(1 for c in both if c.knobs) == 13
    for c in both[16:]:
        knob(c.knobs)
        assert tall_plan(c) == c.plan, (L.case_id(c), c.plan, tall_plan(c))
    assert {c.epi.relu for c in L.tall_cases() if c.why == "nk1" and not c.knobs} == {False, True}


@pytest.mark.parametrize("why", ["seam", "train"])
def test_tall_cases_can_see_four_plausible_bugs(why):
    """The expected bf16 output of the seam case and of the training-shape case differs from what each wrong form would store."""
    for c in [c for c in L.tall_cases() if c.why == why and not c.knobs]:
        want = L.rne_bf16(L.expected(c)[1])
        wrong = L.tall_wrong_forms(c)
        assert len(wrong) == 4
        for name, got in wrong.items():
            n = int((got != want).sum())
            print(f"[lattice] {L.case_id(c)}: '{name}' differs in {n} of {want.numel()} elements")
            if name == "ReLU before the row-group term" and not c.epi.relu:
                assert n == 0                                     # no ReLU: the same thing; the ReLU case of the pair tells
            else:
                assert n >= 1000, (L.case_id(c), name, n)
        # row // 256 is the right group only while the two agree: in the first 256 rows, and nowhere once they have drifted apart
        rows = (wrong["group = row // 256"] != want).any(1)
        assert 0 < int(rows.sum()) < c.M


def test_tall_row_group_arguments_are_refused_before_any_hip_call():
    """The table is read 16 bytes at a time: rg_ld >= N, rg_ld % 4 == 0 and a 16-byte aligned rowgroup, or VQA_ERR_INVALID.
    The pointers are never dereferenced on the host, and a refusal comes before the first HIP call."""
    from dl_vqa_amd import _lib
    lib = _lib.load()
    M, N, K = 2048, 1024, 192
    base = 1 << 20

    def rc(rg, rg_ld):
        return lib.vqa_gemm_tall_bf16(base, K, base, K, base, N, M, N, K, rg, rg_ld, 256, 0, 1, 0, None)
    for rg, rg_ld in ((base, N - 4), (base, N + 2), (base + 4, N)):
        assert rc(rg, rg_ld) == 1, (rg, rg_ld)
        assert b"rowgroup must be 16-byte aligned" in lib.vqa_last_error()
