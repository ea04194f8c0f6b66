"""The ragged XXH32's kernels (ck_ragged.hip) in the built
library's code-object metadata (tests/kernel_meta.py; no GPU): the product and
the chain kernel are there, one instance per sample width, compiled for gfx950
(kernel_meta reads gfx950 code objects only), without VGPR spills and without
scratch.  The chain kernel keeps two batches of 32 x 16 bytes of products in
registers (the look-ahead), so its VGPR count is large by design, 256 to 288:
one wave per workgroup and per SIMD.  The product kernel stays within 64."""
import os

import pytest

import kernel_meta
from conftest import PKG_DIR

LIB = os.path.join(PKG_DIR, "lib", "libairscmp.so")
NAMES = ("ckr_pre_kernel", "ckr_chain_kernel")


@pytest.fixture(scope="module")
def found(prod):
    meta = kernel_meta.kernels(LIB)
    return {want: [k for n, k in meta.items() if want in n] for want in NAMES}


@pytest.mark.parametrize("want", NAMES)
def test_kernel_is_in_the_library_for_both_sample_widths(found, want):
    assert len(found[want]) == 2, (want, [k[".name"] for k in found[want]])


@pytest.mark.parametrize("want", NAMES)
def test_kernel_has_no_spills_or_scratch(found, want):
    assert found[want]
    for k in found[want]:
        print(k[".name"], "vgpr", k[".vgpr_count"], "sgpr", k[".sgpr_count"])
        assert k[".vgpr_spill_count"] == 0, (want, k[".vgpr_spill_count"])
        assert k[".sgpr_spill_count"] == 0, (want, k[".sgpr_spill_count"])
        assert k.get(".private_segment_fixed_size", 0) == 0, want
        assert k.get(".group_segment_fixed_size", 0) == 0, want
        if want == "ckr_pre_kernel":
            # a streaming kernel whose latency occupancy hides: 8 waves per SIMD
            assert k[".vgpr_count"] <= 64, (want, k[".vgpr_count"])
        else:
            # the look-ahead is two batches of 32 x 4 registers and must stay in
            # registers; addresses, accumulator and tail get 32 more at most
            assert 256 <= k[".vgpr_count"] <= 288, (want, k[".vgpr_count"])


def test_the_ragged_encode_kernel_still_has_its_twenty_instances(found):
    """The checksum is a run-time branch of one lane, not a template parameter.
    The ragged instantiations are those of encode_kernel whose tables argument
    is RaggedTabs (its ragged mode)."""
    meta = kernel_meta.kernels(LIB)
    assert len([n for n in meta if "encode_kernel" in n and "RaggedTabs" in n]) == 20
