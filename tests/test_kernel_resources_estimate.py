"""The estimator's kernels (estimate.hip) in the built library's code-object
metadata (tests/kernel_meta.py; no GPU): the sizing kernel for both sample
widths and the finishing kernel are there, compiled for gfx950 (kernel_meta
reads gfx950 code objects only), without spills or scratch.  DESIGN.md 3.8
runs the sizing kernel at three waves per SIMD, 168 VGPRs at the most, with
its accumulators (16 candidates x 256 lanes) and the wave sums in LDS; the
finishing kernel is a streaming sum within 64 VGPRs and uses no LDS."""
import os

import pytest

import kernel_meta
from conftest import PKG_DIR

LIB = os.path.join(PKG_DIR, "lib", "libairscmp.so")
NAMES = {"est_size_kernelILi2E": 168, "est_size_kernelILi4E": 168, "est_finish_kernel": 64}


@pytest.fixture(scope="module")
def est(prod):
    meta = kernel_meta.kernels(LIB)
    return {want: [k for n, k in meta.items() if want in n] for want in NAMES}


@pytest.mark.parametrize("want", sorted(NAMES))
def test_kernel_is_in_the_library_once(est, want):
    assert len(est[want]) == 1, (want, [k[".name"] for k in est[want]])


@pytest.mark.parametrize("want", sorted(NAMES))
def test_kernel_has_no_spills_or_scratch_and_keeps_its_budget(est, want):
    assert est[want]
    for k in est[want]:
        assert k[".vgpr_spill_count"] == 0, (want, k[".vgpr_spill_count"])
        assert k[".sgpr_spill_count"] == 0, (want, k[".sgpr_spill_count"])
        assert k.get(".private_segment_fixed_size", 0) == 0, want
        assert k[".vgpr_count"] + k.get(".agpr_count", 0) <= NAMES[want], (want, k[".vgpr_count"])


def test_lds_of_the_sizing_kernel_allows_three_workgroups_a_cu(est):
    for want in sorted(NAMES)[1:]:
        for k in est[want]:
            # 16 candidates x 256 lanes x 4 bytes, and 16 x 4 wave sums
            assert k[".group_segment_fixed_size"] == 16 * 256 * 4 + 16 * 4 * 4, want
    assert est["est_finish_kernel"][0].get(".group_segment_fixed_size", 0) == 0
