"""The Rice kernel's division by multiplication (csrc/airs_rcp.h, DESIGN.md
3.1.6) on the CPU: tests/rcp/rcp_check.c, a stand-alone C program around the
header, built plain and with AddressSanitizer + UndefinedBehaviorSanitizer and
run directly.  For every frame count 1..4096 and every segments-per-frame
1..511 it compares the multiply form with `/` and `%` for every dividend below
the bound the header documents (d n < 2^32), or below 2^22 where the bound is
larger; it also checks that the host helper returns 0 past the bound, and the
kernel's fallback division against `/`.

The sweep is about 12 G dividends per build, so each build's divisors are
split over a few processes (no GPU, no shared state)."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import PKG_DIR, ROOT

SRC = os.path.join(ROOT, "tests", "rcp", "rcp_check.c")
INC = os.path.join(PKG_DIR, "csrc")
BUILDS = {
    "plain": ["-O2"],
    "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
}
# (verify_asan_link_order=0: the environment may preload a library ahead of the
# program's own ASan runtime; it is left as it is)
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:verify_asan_link_order=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
DCAP = 1 << 22


@pytest.fixture(scope="module", params=sorted(BUILDS))
def prog(request, tmp_path_factory):
    cc = shutil.which("gcc") or shutil.which("cc")
    if not cc:
        pytest.skip("no C compiler")
    out = str(tmp_path_factory.mktemp("rcp") / f"rcp_check_{request.param}")
    r = subprocess.run([cc, "-std=gnu99", "-Wall", "-Wextra", "-Werror", *BUILDS[request.param], "-I", INC, SRC, "-o", out],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


def _expected(lo, hi):
    """dividends per divisor: min(ceil(2^32 / n), 2^22)"""
    return sum(min(((1 << 32) + n - 1) // n, DCAP) for n in range(lo, hi + 1))


def _slices(lo, hi, parts):
    """[lo, hi] cut into `parts` ranges of about equal work"""
    total, cuts, acc, start = _expected(lo, hi), [], 0, lo
    for n in range(lo, hi + 1):
        acc += min(((1 << 32) + n - 1) // n, DCAP)
        if acc >= total * (len(cuts) + 1) / parts or n == hi:
            cuts.append((start, n))
            start = n + 1
    return [c for c in cuts if c[0] <= c[1]]


def _sweep(prog, what, lo, hi):
    parts = max(1, min(8, os.cpu_count() or 1))
    procs = [(a, b, subprocess.Popen([prog, what, str(a), str(b)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                                     text=True, env=ENV)) for a, b in _slices(lo, hi, parts)]
    checked = 0
    for a, b, p in procs:
        out, err = p.communicate(timeout=900)
        assert p.returncode == 0, (what, a, b, out[-500:], err[-3000:])
        assert "runtime error" not in err and "AddressSanitizer" not in err, err[-3000:]
        checked += int(re.search(r"checked (\d+)", out).group(1))
    assert checked == _expected(lo, hi)


def test_frame_counts_1_to_4096(prog):
    _sweep(prog, "nfr", 1, 4096)


def test_segments_per_frame_1_to_511(prog):
    _sweep(prog, "spf", 1, 511)


def test_helper_returns_0_past_the_bound(prog):
    r = subprocess.run([prog, "bound"], capture_output=True, text=True, env=ENV)
    assert r.returncode == 0 and "bound ok" in r.stdout, (r.stdout, r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]


def test_fallback_division(prog):
    r = subprocess.run([prog, "slow"], capture_output=True, text=True, env=ENV)
    assert r.returncode == 0 and "checked" in r.stdout, (r.stdout, r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
