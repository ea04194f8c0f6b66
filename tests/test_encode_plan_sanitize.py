"""The image encoder's host planning under ASan + UBSan, without a device and
without Python in the sanitized process: tests/sanitize/encode_plan_fuzz.c (its
own main) is compiled together with csrc/cmp_image_plan.c -- which must link
alone, with no HIP or device-layer symbol -- and run as a child.  It feeds the
run planner random lists of frame sizes at budgets from less than one frame's
worth upward and checks that every frame lies in exactly one run, the runs are
in order and uniform in size, the budget is kept except by single-frame runs
and the count limit is kept."""
import os
import shutil
import subprocess

import pytest

from conftest import PKG_DIR, ROOT

SRC = os.path.join(PKG_DIR, "csrc", "cmp_image_plan.c")
MAIN = os.path.join(ROOT, "tests", "sanitize", "encode_plan_fuzz.c")


@pytest.fixture(scope="module")
def fuzz(tmp_path_factory):
    if not shutil.which("gcc"):
        pytest.skip("gcc not available")
    exe = str(tmp_path_factory.mktemp("encode_plan") / "encode_plan_fuzz")
    r = subprocess.run(["gcc", "-std=gnu99", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                        "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG_DIR, "csrc"), MAIN, SRC,
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_run_planner_links_alone_and_survives_the_fuzz(fuzz):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:verify_asan_link_order=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([fuzz], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    assert "encode_plan_fuzz: OK" in r.stdout
