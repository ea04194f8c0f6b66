"""The image encoder's kernels (encode_image.hip) in the built library's
code-object metadata (tests/kernel_meta.py; no GPU): the ingest, the offset
scan and the emit kernel are there, compiled for gfx950 (kernel_meta reads
gfx950 code objects only), without spills or scratch, at most 64 VGPRs each.
The two copies are streaming kernels whose latency is hidden by occupancy and
use no LDS; the scan is one workgroup that does."""
import os

import pytest

import kernel_meta
from conftest import PKG_DIR

LIB = os.path.join(PKG_DIR, "lib", "libairscmp.so")
NAMES = ("encimage_ingest_kernel", "encimage_emit_kernel", "encimage_scan_kernel")


@pytest.fixture(scope="module")
def image(prod):
    meta = kernel_meta.kernels(LIB)
    return {want: [k for n, k in meta.items() if want in n] for want in NAMES}


@pytest.mark.parametrize("want", NAMES)
def test_kernel_is_in_the_library_once(image, want):
    assert len(image[want]) == 1, (want, [k[".name"] for k in image[want]])


@pytest.mark.parametrize("want", NAMES)
def test_kernel_has_no_spills_or_scratch(image, want):
    assert image[want]
    for k in image[want]:
        assert k[".vgpr_spill_count"] == 0, (want, k[".vgpr_spill_count"])
        assert k[".sgpr_spill_count"] == 0, (want, k[".sgpr_spill_count"])
        assert k.get(".private_segment_fixed_size", 0) == 0, want
        assert k[".vgpr_count"] <= 64, (want, k[".vgpr_count"])


@pytest.mark.parametrize("want", NAMES[:2])
def test_copy_kernels_use_no_lds(image, want):
    assert image[want]
    for k in image[want]:
        assert k.get(".group_segment_fixed_size", 0) == 0, want
