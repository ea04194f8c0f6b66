"""The layout of the ragged checksum's products (cmp_image_ck_layout,
DESIGN.md 3.4.6) under ASan + UBSan, without a device and without Python in the
sanitized process: tests/sanitize/ragged_ck_layout_fuzz.c (its own main) is
compiled together with csrc/cmp_image_plan.c -- which must link alone, with no
HIP or device-layer symbol -- and run as a child.  The program's header says
what it checks: 16-byte aligned offsets, regions that do not overlap, hold the
frame's products and take at most 2 n + 128 bytes, the total the caller
allocates, the product workgroups, and the sizes at which sums could overflow."""
import os
import shutil
import subprocess

import pytest

from conftest import PKG_DIR, ROOT

SRC = os.path.join(PKG_DIR, "csrc", "cmp_image_plan.c")
MAIN = os.path.join(ROOT, "tests", "sanitize", "ragged_ck_layout_fuzz.c")


@pytest.fixture(scope="module")
def fuzz(tmp_path_factory):
    if not shutil.which("gcc"):
        pytest.skip("gcc not available")
    exe = str(tmp_path_factory.mktemp("ragged_ck_layout") / "ragged_ck_layout_fuzz")
    r = subprocess.run(["gcc", "-std=gnu99", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                        "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG_DIR, "csrc"), MAIN, SRC,
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_layout_links_alone_and_survives_the_fuzz(fuzz):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:verify_asan_link_order=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([fuzz], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    assert "ragged_ck_layout_fuzz: OK" in r.stdout
