"""The stretch between the Rice kernels' entry and their first sample load
(DESIGN.md 3.1.6), read from the built library with scripts/isa_count.py
--front (no GPU): for each of the three Rice kernel variants that
test_kernel_resources.py lists, in text order before the first vector-memory
load, there is no reciprocal division (v_rcp_iflag_f32) and there are at most
two `s_waitcnt lgkmcnt(0)`: the front block's, and the one of the
frame_list[lf] read.  Before the front block there were four waits and two
divisions."""
import os
import re
import subprocess
import sys

import pytest

from conftest import PKG_DIR

ROOT = os.path.dirname(PKG_DIR)
LIB = os.path.join(PKG_DIR, "lib", "libairscmp.so")
SYMS = {
    "frame DIFF": "_ZN4airs11rice_kernelILi1ELb0ELb0EEEvNS_5KArgsE",
    "frame NONE": "_ZN4airs11rice_kernelILi0ELb0ELb0EEEvNS_5KArgsE",
    "stream DIFF": "_ZN4airs11rice_kernelILi1ELb1ELb0EEEvNS_5KArgsE",
    "auto DIFF": "_ZN4airs11rice_kernelILi1ELb0ELb1EEEvNS_5KArgsE",
    "auto NONE": "_ZN4airs11rice_kernelILi0ELb0ELb1EEEvNS_5KArgsE",
}


def _front(sym):
    if not os.path.exists(LIB):
        pytest.skip("libairscmp.so not built")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "isa_count.py"), sym, LIB, "--front"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.split("entry .. first vector-memory load (text order)\n")[1].split("\n\n")[0].splitlines()
    ins = [ln.strip() for ln in lines if ln.startswith("  ")]
    return ins, r.stdout


@pytest.mark.parametrize("name", sorted(SYMS))
def test_front_chain(name):
    ins, out = _front(SYMS[name])
    # the listing ends with the first vector-memory load, a sample load
    assert re.match(r"^(global|buffer|flat)_load", ins[-1]), ins[-1]
    assert ins[-1].startswith("global_load_dwordx4"), ins[-1]
    before = ins[:-1]
    assert not [i for i in before if i.startswith("v_rcp")], out
    waits = [i for i in before if i.startswith("s_waitcnt")]
    assert all(re.fullmatch(r"s_waitcnt lgkmcnt\(0\)", w) for w in waits), waits
    assert len(waits) <= 2, out
    # one read of the kernel-argument segment, the front block's 64 bytes; the
    # only other scalar load is the frame list entry
    loads = [i for i in before if i.startswith("s_load")]
    assert loads[0].startswith("s_load_dwordx16") and loads[0].endswith("0x0"), loads
    assert len(loads) <= 2 and all(ld.startswith("s_load_dword ") for ld in loads[1:]), loads
    # and the summary the script prints agrees with the listing
    m = re.search(r"s_waitcnt\s+(\d+)\n\s+v_rcp_iflag_f32\s+(\d+)", out)
    assert m and int(m.group(1)) == len(waits) and int(m.group(2)) == 0, out
