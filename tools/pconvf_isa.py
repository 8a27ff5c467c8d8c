#!/usr/bin/env python3
"""The stage loop of pconvf_dgrad_kernel (csrc/conv_patch_f32.hip) as hipcc built it, read from the library's gfx950 code
objects (no GPU needed):
    python tools/pconvf_isa.py [dl_vqa_amd/libvqa_hip.so] > profiles/pconvf_tail_isa.txt
A k-step of a tile of NI row blocks is 2 NI MFMAs on fragments that were read a whole k-step earlier.  For every kernel and
every NI the summary counts the k-steps whose MFMAs issue back to back (nothing between them, no wait inside the group) and
the LDS reads and waits in front of such a group.  The full tile (NI = 4, 8 MFMAs) is the hot one: three reads (the four A
fragments as two ds_read2_b32, the two B fragments as one) and one wait per k-step is the schedule the measured speed rests
on (profiles/pconvf_tail_timing.txt); tests/test_pconvf_isa_cpu.py holds the built library to it."""
import os
import re
import struct
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
KERNELS = {8: "_ZN3vqa19pconvf_dgrad_kernelILi8EEEvNS_8PfParamsE", 4: "_ZN3vqa19pconvf_dgrad_kernelILi4EEEvNS_8PfParamsE"}


def code_objects(path, td):
    """the gfx950 code objects of a shared library, as files under td"""
    fat = os.path.join(td, "fat.bin")
    subprocess.run([f"{LLVM}/llvm-objcopy", "--dump-section", f".hip_fatbin={fat}", path, os.path.join(td, "copy")],
                   check=True, capture_output=True)
    data = open(fat, "rb").read()
    out = []
    for bi, m in enumerate(re.finditer(re.escape(b"__CLANG_OFFLOAD_BUNDLE__"), data)):
        p = m.start()
        n = struct.unpack_from("<Q", data, p + 24)[0]
        off = p + 32
        for _ in range(n):
            eoff, esize, tlen = struct.unpack_from("<QQQ", data, off)
            off += 24
            triple = data[off:off + tlen].decode()
            off += tlen
            if "gfx950" in triple and esize:
                co = os.path.join(td, f"co{bi}.elf")
                open(co, "wb").write(data[p + eoff:p + eoff + esize])
                out.append(co)
    return out


def mnemonics(path, symbol):
    """the instruction mnemonics of one kernel, in program order"""
    with tempfile.TemporaryDirectory() as td:
        for co in code_objects(path, td):
            if symbol.encode() not in open(co, "rb").read():
                continue
            txt = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", f"--disassemble-symbols={symbol}", co],
                                 capture_output=True, text=True).stdout
            ins = [m.group(1) for m in re.finditer(r"^\s+([a-z][a-z0-9_]+)\b.*//", txt, flags=re.M)]
            if ins:
                return ins
    raise RuntimeError(f"{symbol} not found in {path}")


def ksteps(ins):
    """{MFMAs per group: (groups issued back to back, LDS reads in front of them, waits in front of them, groups in all)}: a
    group is a maximal run of MFMAs with nothing between them; `in all` also counts the runs a wait or anything else cuts"""
    runs, gap, i = [], [], 0
    while i < len(ins):
        if ins[i].startswith("v_mfma"):
            j = i
            while j < len(ins) and ins[j].startswith("v_mfma"):
                j += 1
            runs.append((j - i, gap))
            gap, i = [], j
        else:
            gap.append(ins[i])
            i += 1
    out = {}
    for n in (2, 4, 6, 8):
        mine = [g for k, g in runs if k == n]
        out[n] = (len(mine), sum(x.startswith("ds_read") for g in mine for x in g), sum(x == "s_waitcnt" for g in mine for x in g))
    return out, len(runs)


def summary(path):
    lines = []
    for wm, sym in KERNELS.items():
        ins = mnemonics(path, sym)
        ks, nruns = ksteps(ins)
        lines.append(f"pconvf_dgrad_kernel<{wm}>: {len(ins)} instructions, {sum(x.startswith('v_mfma') for x in ins)} MFMAs in {nruns} runs")
        for n, (groups, reads, waits) in ks.items():
            per = f"{reads / groups:.2f} LDS reads, {waits / groups:.2f} waits per k-step" if groups else "-"
            lines.append(f"    NI = {n // 2}: {groups:4d} k-steps of {n} MFMAs back to back; in front of them {reads} LDS reads, {waits} waits = {per}")
    return lines


if __name__ == "__main__":
    lib = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                             "dl_vqa_amd", "libvqa_hip.so")
    print("\n".join(summary(lib)))
