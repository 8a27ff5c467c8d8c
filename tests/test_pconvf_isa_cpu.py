"""The full-tile stage loop of pconvf_dgrad_kernel as hipcc built it (no GPU: read from the library's code objects).

The kernel's measured speed (profiles/pconvf_tail_timing.txt) rests on a schedule that nothing in the source pins: in a full
tile (NI = 4) every one of the 36 k-steps of a stage issues its 8 MFMAs back to back, behind three LDS reads -- the four A
fragments as two ds_read2_b32, the two B fragments as one -- that were issued a whole k-step earlier.  An earlier build read
the B fragments one by one and put a second wait behind the first MFMA of every k-step, and was 2-3 % slower for it
(profiles/pconvf_tail_isa.txt).  An edit or a compiler that loses this should be seen here, not in a later benchmark."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("wm", [8, 4])
def test_full_tile_ksteps_issue_back_to_back_behind_three_lds_reads(wm):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from pconvf_isa import KERNELS, ksteps, mnemonics
    from dl_vqa_amd import _lib, build
    build.build_library(verbose=False)
    ks, _ = ksteps(mnemonics(_lib.LIB_PATH, KERNELS[wm]))
    groups, reads, _ = ks[8]
    print(f"pconvf_dgrad_kernel<{wm}>: {groups} full-tile k-steps back to back, {reads} LDS reads in front of them")
    assert groups >= 36 and groups % 36 == 0, "a full-tile k-step is cut: its 8 MFMAs no longer issue back to back"
    assert reads <= 3 * groups, "more than three LDS reads per full-tile k-step: the fragment reads are no longer paired"
