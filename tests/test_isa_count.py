"""scripts/isa_count.py on the built library (no GPU): the Rice frame kernel's
instruction accounting parses, its classes add up, its metadata is the code
object's, and the fixed work of DESIGN.md 3.1.5 stays where that section puts
it: few vector instructions between B1 and the packer, no spill moves on the
common path beyond the look-back's two."""
import os
import re
import subprocess
import sys

import pytest

import kernel_meta
from conftest import PKG_DIR

ROOT = os.path.dirname(PKG_DIR)
LIB = os.path.join(PKG_DIR, "lib", "libairscmp.so")
SYM = "_ZN4airs11rice_kernelILi1ELb0ELb0EEEvNS_5KArgsE"


@pytest.fixture(scope="module")
def report():
    if not os.path.exists(LIB):
        pytest.skip("libairscmp.so not built")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "isa_count.py"), SYM, LIB, "--split",
                        "s_setprio"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return r.stdout


def _rows(report, head):
    rows, on = {}, False
    for ln in report.splitlines():
        if ln.startswith(head):
            on = True
        elif on and not ln.strip():
            break
        elif on:
            m = re.match(r"^\s*(?:\d+ )?(.+?)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)$", ln)
            assert m, ln
            rows[m.group(1).strip()] = [int(v) for v in m.groups()[1:]]
    return rows


def test_isa_count_regions_and_blocks_add_up(report):
    regions = _rows(report, "region   ")
    blocks = _rows(report, "region block")
    whole = regions.pop("whole kernel")
    assert all(sum(r[:5]) == r[5] for r in regions.values())
    assert [sum(r[i] for r in regions.values()) for i in range(6)] == whole
    assert [sum(b[i] for b in blocks.values()) for i in range(6)] == whole
    # the kernel's barriers in text order, and the packer's start
    assert "entry..B0" in regions and "B0..B1" in regions and "B1..s_setprio" in regions
    assert whole[0] > 1000 and whole[1] > 1000 and whole[2] > 100 and whole[3] > 10


def test_isa_count_metadata_is_the_code_objects(report):
    meta = kernel_meta.kernels(LIB)[SYM]
    for key in (".vgpr_count", ".sgpr_spill_count", ".vgpr_spill_count", ".private_segment_fixed_size"):
        m = re.search(r"^\s+" + re.escape(key[1:]) + r"\s+(\d+)$", report, re.M)
        assert m and int(m.group(1)) == meta[key], key


def test_rice_fixed_work_stays_scalar(report):
    """22 vector instructions between B1 and the packer (53
    before the wave totals moved to scalar code; the plan's aim: at most ~25,
    a margin of five for the toolchain), and two SGPR spills (19 before)."""
    regions = _rows(report, "region   ")
    assert regions["B1..s_setprio"][0] <= 30, regions["B1..s_setprio"]
    assert kernel_meta.kernels(LIB)[SYM][".sgpr_spill_count"] <= 4
