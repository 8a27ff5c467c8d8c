"""CPU: the host rules that vqa_gemm, vqa_gemm_x3 and vqa_gemm_bf16 share (csrc/gemm_host.hpp) -- argument check, split-K
workspace claim and the planners behind *_workspace_bytes.  Every check here returns before the first HIP call; the operands
are made-up 16-byte-aligned integers that nothing dereferences.

The PLAN table holds what the library of the commit BEFORE the host code was folded reported, not what this tree computes.
It was printed by this module run against that commit's library, with no VQA_* knob in the environment:

    VQA_LIB=<checkout of the parent commit>/dl_vqa_amd/libvqa_hip.so python -m tests.test_gemm_host_cpu
"""
import os

import pytest

A, B, C, WS, RG = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000
OK, INVALID, WORKSPACE = 0, 1, 3
ENGINES = ("vqa_gemm", "vqa_gemm_x3", "vqa_gemm_bf16")
QUANTUM = {"vqa_gemm": 4, "vqa_gemm_x3": 4, "vqa_gemm_bf16": 8}      # elements per 16 bytes

# (M, N, K) by planner arm.  fp32 / bf16 (plan_gemm, 32 / 64 elements a K-step, 512 resident slots):
SHAPES = [
    # 200 or more 128 x 128 tiles: no split, or target / tiles splits where 2 x tiles still fit and K has >= 64 steps
    (2048, 2048, 512), (4096, 4096, 4096), (4096, 4096, 64), (2048, 2048, 2048), (2048, 2048, 4096), (1920, 1920, 4096),
    (1800, 1900, 8200), (2048, 2048, 2016), (3000, 1100, 5000),
    # fewer, but 200 or more 64 x 64 tiles
    (1024, 1024, 4096), (896, 1024, 8192), (1000, 900, 333), (8192, 128, 4096),
    # few tiles, 64 x 64: splits from the slot target, the K-steps / 4 cap, the 64 cap
    (256, 1024, 2560), (250, 1000, 2500), (256, 2048, 1024), (64, 64, 256), (128, 128, 100000), (100, 3000, 1280),
    (333, 777, 5000), (512, 512, 512), (8, 8, 10000), (640, 256, 8192),
    # few tiles, 128 x 128: every split keeps 16 or more K-steps
    (512, 256, 173056), (1024, 256, 66008), (384, 256, 66008), (1024, 256, 173056), (256, 256, 40000), (1024, 1024, 65536),
    (130, 1000, 200000),
    # one K-step
    (64, 64, 32), (300, 200, 16), (256, 1024, 64),
    # x3 (192 x 128 tiles, 256 slots): 128 or more tiles, fewer, the K-steps / 8 cap, the 64 cap
    (3072, 1024, 256), (2880, 1024, 256), (192, 128, 100000), (1536, 1024, 2048), (200, 130, 1000), (2304, 1024, 8192),
]

# name -> {(M, N, K): bytes}; see the module docstring
PLAN = {
    "vqa_gemm": {
        (2048, 2048, 512): 0, (4096, 4096, 4096): 0, (4096, 4096, 64): 0, (2048, 2048, 2048): 33554432,
        (2048, 2048, 4096): 33554432, (1920, 1920, 4096): 29491200, (1800, 1900, 8200): 27360000, (2048, 2048, 2016): 0,
        (3000, 1100, 5000): 26400000, (1024, 1024, 4096): 0, (896, 1024, 8192): 0, (1000, 900, 333): 0,
        (8192, 128, 4096): 0, (256, 1024, 2560): 8388608, (250, 1000, 2500): 8000000, (256, 2048, 1024): 8388608,
        (64, 64, 256): 32768, (128, 128, 100000): 4194304, (100, 3000, 1280): 6000000, (333, 777, 5000): 6209784,
        (512, 512, 512): 4194304, (8, 8, 10000): 16128, (640, 256, 8192): 7864320, (512, 256, 173056): 33554432,
        (1024, 256, 66008): 33554432, (384, 256, 66008): 24772608, (1024, 256, 173056): 33554432,
        (256, 256, 40000): 8388608, (1024, 1024, 65536): 0, (130, 1000, 200000): 16640000, (64, 64, 32): 0,
        (300, 200, 16): 0, (256, 1024, 64): 0, (3072, 1024, 256): 0, (2880, 1024, 256): 0, (192, 128, 100000): 6291456,
        (1536, 1024, 2048): 0, (200, 130, 1000): 832000, (2304, 1024, 8192): 0,
    },
    "vqa_gemm_x3": {
        (2048, 2048, 512): 0, (4096, 4096, 4096): 0, (4096, 4096, 64): 0, (2048, 2048, 2048): 0, (2048, 2048, 4096): 0,
        (1920, 1920, 4096): 0, (1800, 1900, 8200): 0, (2048, 2048, 2016): 0, (3000, 1100, 5000): 0,
        (1024, 1024, 4096): 20971520, (896, 1024, 8192): 22020096, (1000, 900, 333): 0, (8192, 128, 4096): 20971520,
        (256, 1024, 2560): 10485760, (250, 1000, 2500): 9000000, (256, 2048, 1024): 8388608, (64, 64, 256): 0,
        (128, 128, 100000): 4194304, (100, 3000, 1280): 6000000, (333, 777, 5000): 18629352, (512, 512, 512): 2097152,
        (8, 8, 10000): 8960, (640, 256, 8192): 20971520, (512, 256, 173056): 22020096, (1024, 256, 66008): 22020096,
        (384, 256, 66008): 24772608, (1024, 256, 173056): 22020096, (256, 256, 40000): 16515072,
        (1024, 1024, 65536): 20971520, (130, 1000, 200000): 16640000, (64, 64, 32): 0, (300, 200, 16): 0,
        (256, 1024, 64): 0, (3072, 1024, 256): 0, (2880, 1024, 256): 0, (192, 128, 100000): 6291456,
        (1536, 1024, 2048): 25165824, (200, 130, 1000): 416000, (2304, 1024, 8192): 18874368,
    },
    "vqa_gemm_bf16": {
        (2048, 2048, 512): 0, (4096, 4096, 4096): 0, (4096, 4096, 64): 0, (2048, 2048, 2048): 0,
        (2048, 2048, 4096): 33554432, (1920, 1920, 4096): 29491200, (1800, 1900, 8200): 27360000, (2048, 2048, 2016): 0,
        (3000, 1100, 5000): 26400000, (1024, 1024, 4096): 0, (896, 1024, 8192): 0, (1000, 900, 333): 0,
        (8192, 128, 4096): 0, (256, 1024, 2560): 8388608, (250, 1000, 2500): 8000000, (256, 2048, 1024): 8388608,
        (64, 64, 256): 0, (128, 128, 100000): 4128768, (100, 3000, 1280): 6000000, (333, 777, 5000): 6209784,
        (512, 512, 512): 2097152, (8, 8, 10000): 8192, (640, 256, 8192): 7864320, (512, 256, 173056): 33030144,
        (1024, 256, 66008): 33554432, (384, 256, 66008): 8257536, (1024, 256, 173056): 33554432,
        (256, 256, 40000): 8388608, (1024, 1024, 65536): 0, (130, 1000, 200000): 16640000, (64, 64, 32): 0,
        (300, 200, 16): 0, (256, 1024, 64): 0, (3072, 1024, 256): 0, (2880, 1024, 256): 0, (192, 128, 100000): 6193152,
        (1536, 1024, 2048): 0, (200, 130, 1000): 416000, (2304, 1024, 8192): 0,
    },
}


def _lib():
    from dl_vqa_amd import _lib
    return _lib.load()


@pytest.fixture()
def lib(monkeypatch):
    """The library with no VQA_* knob in force (the knobs are read once per process, other tests may have set some)."""
    for k in [k for k in os.environ if k.startswith("VQA_") and k != "VQA_LIB"]:
        monkeypatch.delenv(k)
    lib = _lib()
    lib.vqa_reload_knobs()
    yield lib
    monkeypatch.undo()
    lib.vqa_reload_knobs()


def _call(lib, name, M, N, K, *, a=A, lda=None, transA=0, ldb=None, transB=1, ldc=None, c_is_bf16=0, rowgroup=None, rg_div=1,
          accumulate=0, ws=None, ws_bytes=0):
    lda = lda if lda is not None else (M if transA else K)
    ldb = ldb if ldb is not None else (K if transB else N)
    ldc = ldc if ldc is not None else N
    kind = (c_is_bf16,) if name == "vqa_gemm_bf16" else ()
    rc = getattr(lib, name)(a, lda, transA, B, ldb, transB, C, ldc, *kind, M, N, K, None, None, rowgroup, N, rg_div, 0, 0,
                            accumulate, None, ws, ws_bytes, 0, None)
    return rc, lib.vqa_last_error()


@pytest.mark.parametrize("name", ENGINES)
def test_workspace_claim(lib, name):
    M, N, K = 256, 1024, 2560
    need = getattr(lib, name + "_workspace_bytes")(M, N, K)
    assert need > 0 and need % (M * N * 4) == 0
    for ws, ws_bytes in ((None, 0), (None, need), (WS, need - 1)):
        rc, msg = _call(lib, name, M, N, K, ws=ws, ws_bytes=ws_bytes)
        assert rc == WORKSPACE, (rc, msg)
        assert msg.startswith(name.encode() + b": workspace ") and f"< {need} needed".encode() in msg, msg


@pytest.mark.parametrize("name", ENGINES)
def test_argument_errors(lib, name):
    q = QUANTUM[name]
    M, N, K = 256, 1024, 2560
    cases = {
        "misaligned A": (dict(a=A + 4), b"16-byte"),
        "lda off the quantum": (dict(lda=K + q // 2), b"16-byte"),
        "lda = 2^21": (dict(lda=1 << 21), b"2^21"),
        "ldb = 2^21": (dict(ldb=1 << 21), b"2^21"),
        "ldc = 2^21": (dict(ldc=1 << 21), b"2^21"),
        "rowgroup without rg_div": (dict(rowgroup=RG, rg_div=0), b"rg_div"),
    }
    for what, (kw, fragment) in cases.items():
        rc, msg = _call(lib, name, M, N, K, ws=WS, ws_bytes=1 << 40, **kw)
        assert rc == INVALID and msg.startswith(name.encode() + b":") and fragment in msg, (what, rc, msg)
    if name == "vqa_gemm_bf16":
        for what, (m, n, k, kw, fragment) in {
            "K % 8": (M, N, K + 4, dict(lda=K + 8, ldb=K + 8), b"K=2564"),
            "reduction-major A, M % 8": (M + 4, N, K, dict(transA=1, lda=M + 8), b"reduction-major"),
            "reduction-major B, N % 8": (M, N + 4, K, dict(transB=0, ldb=N + 8, ldc=N + 8), b"reduction-major"),
            "bf16 C with accumulate": (M, N, K, dict(c_is_bf16=1, accumulate=1), b"fp32 C"),
        }.items():
            rc, msg = _call(lib, name, m, n, k, ws=WS, ws_bytes=1 << 40, **kw)
            assert rc == INVALID and msg.startswith(b"vqa_gemm_bf16:") and fragment in msg, (what, rc, msg)


@pytest.mark.parametrize("name", ENGINES)
def test_plan_table(lib, name):
    table = PLAN[name]
    assert len(table) >= 30 and set(table) == set(SHAPES)
    got = {s: getattr(lib, name + "_workspace_bytes")(*s) for s in table}
    assert got == table, {s: (got[s], table[s]) for s in table if got[s] != table[s]}
    assert 0 in table.values() and len(set(table.values())) > 10      # split and unsplit plans are both in the table


if __name__ == "__main__":
    assert not [k for k in os.environ if k.startswith("VQA_") and k != "VQA_LIB"], "unset every VQA_* knob first"
    print("PLAN = {")
    for name in ENGINES:
        print(f'    "{name}": {{')
        row = ""
        for s in SHAPES:
            item = f"{s}: {getattr(_lib(), name + '_workspace_bytes')(*s)}, "
            if len(row) + len(item) > 116:
                print("        " + row.rstrip())
                row = ""
            row += item
        print("        " + row.rstrip())
        print("    },")
    print("}")
