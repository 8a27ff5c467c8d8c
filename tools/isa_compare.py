#!/usr/bin/env python3
"""Kernel by kernel, is the device code of two builds of the library the same?  Reads the gfx950 code objects of both (no GPU
needed), disassembles them with llvm-objdump and compares every kernel's instruction sequence -- mnemonics and operands, in
program order -- and its VGPRs, SGPRs, scratch and LDS from the code objects' metadata:
    python tools/isa_compare.py PARENT_LIB BRANCH_LIB [--rename OLD=NEW ...] > profiles/NAME_isa.txt
--rename: a parent kernel that the branch builds under another name.  OLD is a regular expression over the parent's (mangled)
kernel names and NEW its replacement, as in re.sub; a whole name works as it is.  @FILE reads arguments from FILE, one per line
(--rename=OLD=NEW).  One line per kernel, then the counts.  The exit status is 1 if a kernel outside the rename map was added,
removed or changed, or if a renamed pair differs."""
import argparse
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pconvf_isa import LLVM, code_objects  # noqa: E402


def kernels(lib):
    """{kernel symbol: (vgpr, sgpr, scratch, lds, [instruction text])} of every gfx950 kernel of a library"""
    out = {}
    with tempfile.TemporaryDirectory() as td:
        for co in code_objects(lib, td):
            notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], check=True, capture_output=True, text=True).stdout
            meta = {}
            for entry in notes.split(".wavefront_size:")[:-1]:           # a kernel's keys are sorted: this one is its last
                sym = re.findall(r"\.symbol:\s+'?([^\s']+)\.kd", entry)[-1]
                g = lambda key: int(re.findall(key + r":\s+(\d+)", entry)[-1])
                meta[sym] = (g(r"\.vgpr_count"), g(r"\.sgpr_count"), g(r"\.private_segment_fixed_size"), g(r"\.group_segment_fixed_size"))
            dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", co], check=True, capture_output=True, text=True).stdout
            cur = None
            for line in dis.splitlines():
                m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
                if m:
                    cur = out.setdefault(m.group(1), meta[m.group(1)] + ([],))[4] if m.group(1) in meta else None
                elif cur is not None and line[:1] in " \t" and line.strip():
                    cur.append(" ".join(line.split("//")[0].split()))
    for k in out.values():                                               # what follows the last s_endpgm pads the next function's start
        ins = k[4]
        if "s_endpgm" in ins:
            del ins[len(ins) - ins[::-1].index("s_endpgm"):]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0], fromfile_prefix_chars="@")
    ap.add_argument("parent")
    ap.add_argument("branch")
    ap.add_argument("--rename", action="append", default=[], metavar="OLD=NEW")
    args = ap.parse_args()
    old, new = kernels(args.parent), kernels(args.branch)
    renamed = {}                                                         # branch name: parent name
    for r in args.rename:
        pat, rep = r.split("=", 1)
        for name in old:
            if re.fullmatch(pat, name):
                renamed[re.sub(pat, rep, name)] = name
    pairs = [(renamed.get(n, n), n) for n in new if renamed.get(n, n) in old]
    taken = {o for o, _ in pairs}
    added = sorted(n for n in new if renamed.get(n, n) not in old)
    removed = sorted(o for o in old if o not in taken)
    print("columns: parent/branch; `same` = the instruction sequence (mnemonics and operands) is identical")
    same = 0
    for o, n in sorted(pairs, key=lambda p: p[1]):
        a, b = old[o], new[n]
        ok = a == b
        same += ok
        print(f"{'same' if ok else 'DIFF'} vgpr {a[0]:3d}/{b[0]:3d} sgpr {a[1]:3d}/{b[1]:3d} scratch {a[2]}/{b[2]} lds {a[3]}/{b[3]} "
              f"insts {len(a[4])}/{len(b[4])} {n}" + (f"  (parent: {o})" if o != n else ""))
    for n in added:
        print(f"added   {n}")
    for o in removed:
        print(f"removed {o}")
    print(f"kernels compared {len(pairs)} (renamed {sum(o != n for o, n in pairs)}); identical {same}; added {len(added)}; "
          f"removed {len(removed)}")
    return 0 if same == len(pairs) and not added and not removed else 1


if __name__ == "__main__":
    sys.exit(main())
