"""The batch planner behind cmp_gpu_compress plans as recorded.

tests/sanitize/host_fuzz.c drives the planner over the host-memory device stub
(tests/sanitize/dev_stub.c) and prints three 64-bit digests for a seed:
  result   what every batch call returned (sizes, draws, frame heads, contexts)
  launch   what the planner handed to the device layer: every field of every
           encode / walk / fb_step / fb_copy / checksum / patch / commit call,
           and per launched frame the identifier, sequence number, model place
           and checksum the device would resolve
  traffic  scratch requests, copies and synchronisations, in call order
tests/planner_digest.json holds them for five runs.  A change to the planner's
host code that is meant to leave the plan alone (a refactor) must leave all
fifteen values as they are.

To regenerate the file: build the harness and run it for each (iterations,
seed) of the file,
    make -C tests/sanitize host_fuzz && tests/sanitize/host_fuzz 5000 1
and copy the three digests it prints.  `make -C tests/sanitize host_fuzz
HOST_SRC=<path to another tree's cmp_host.c ...>` builds the same harness
against another tree's planner sources, which is how the file was recorded: from
the planner as it was before it moved to cmp_batch.c.  A pull request that
changes the plan on purpose regenerates the file and says so."""
import json
import os
import re
import shutil
import subprocess

import pytest

TESTS = os.path.dirname(os.path.abspath(__file__))
HERE = os.path.join(TESTS, "sanitize")

with open(os.path.join(TESTS, "planner_digest.json")) as _f:
    RUNS = json.load(_f)["runs"]


@pytest.fixture(scope="module")
def fuzz_bin():
    if not shutil.which("gcc"):
        pytest.skip("gcc not available")
    r = subprocess.run(["make", "-s", "-C", HERE, "host_fuzz"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return os.path.join(HERE, "host_fuzz")


@pytest.mark.parametrize("run", RUNS, ids=lambda r: f"seed{r['seed']}x{r['iterations']}")
def test_planner_digests(fuzz_bin, run):
    # the environment of tests/test_sanitize_cpu.py, nothing more
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1:verify_asan_link_order=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([fuzz_bin, str(run["iterations"]), str(run["seed"])], capture_output=True, text=True,
                       errors="replace", env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    m = re.search(r"walks, digest ([0-9a-f]{16})\nlaunch digest ([0-9a-f]{16}), traffic digest ([0-9a-f]{16})", r.stdout)
    assert m, r.stdout
    print("result %s launch %s traffic %s" % m.groups())
    assert m.group(1) == run["result"]
    assert m.group(2) == run["launch"]
    assert m.group(3) == run["traffic"]
