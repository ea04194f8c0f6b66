"""The XXH32 kernels (checksum.hip) in the built
library's code-object metadata (tests/kernel_meta.py; no GPU): the product and
the chain kernel of both layouts are there, the ragged ones with one instance
per sample width, the strided ones with one per sample width and frame-size
mode (VN), compiled for gfx950 (kernel_meta reads gfx950 code objects only),
without VGPR spills, scratch or LDS.  A chain kernel keeps two batches of
32 x 16 bytes of products in registers (the look-ahead), so its VGPR count is
large by design, 256 to 288: one wave per workgroup and per SIMD.  A product
kernel stays within 64.

The strided kernels also have a ceiling per instance (PARENT_VGPRS): the VGPR
count read from the build of commit 8d35462, the last one that had them in
encode.hip.  There ck_pre_kernel's four were all in the occupancy step that
ends at 64 (8 waves per SIMD), and ck_chain_kernel's took the two batches (256)
and 8 to 12 more."""
import os

import pytest

import kernel_meta
from conftest import PKG_DIR

LIB = os.path.join(PKG_DIR, "lib", "libairscmp.so")
INSTANCES = {"ckr_pre_kernel": 2, "ckr_chain_kernel": 2, "ck_pre_kernel": 4, "ck_chain_kernel": 4}
NAMES = tuple(INSTANCES)
# (kernel, sample bytes, VN) -> VGPRs in the build of commit 8d35462
PARENT_VGPRS = {("ck_pre_kernel", 2, 0): 32, ("ck_pre_kernel", 2, 1): 34, ("ck_pre_kernel", 4, 0): 46,
                ("ck_pre_kernel", 4, 1): 47, ("ck_chain_kernel", 2, 0): 264, ("ck_chain_kernel", 2, 1): 268,
                ("ck_chain_kernel", 4, 0): 264, ("ck_chain_kernel", 4, 1): 268}


def instance(want, w, vn):
    """The mangled template arguments: ILi<W>E for the ragged kernels, ILi<W>ELb<VN>E for the strided."""
    return "%sILi%dELb%dE" % (want, w, vn)


@pytest.fixture(scope="module")
def found(prod):
    meta = kernel_meta.kernels(LIB)
    return {want: [k for n, k in meta.items() if want in n] for want in NAMES}


@pytest.mark.parametrize("want", NAMES)
def test_kernel_is_in_the_library_for_both_sample_widths(found, want):
    assert len(found[want]) == INSTANCES[want], (want, [k[".name"] for k in found[want]])
    for w in (2, 4):
        if INSTANCES[want] == 2:
            assert len([k for k in found[want] if "%sILi%dEEE" % (want, w) in k[".name"]]) == 1, (want, w)
        else:  # both frame-size modes of each width
            for vn in (0, 1):
                assert len([k for k in found[want] if instance(want, w, vn) in k[".name"]]) == 1, (want, w, vn)


@pytest.mark.parametrize("want", NAMES)
def test_kernel_has_no_spills_or_scratch(found, want):
    assert found[want]
    for k in found[want]:
        print(k[".name"], "vgpr", k[".vgpr_count"], "sgpr", k[".sgpr_count"])
        assert k[".vgpr_spill_count"] == 0, (want, k[".vgpr_spill_count"])
        assert k[".sgpr_spill_count"] == 0, (want, k[".sgpr_spill_count"])
        assert k.get(".private_segment_fixed_size", 0) == 0, want
        assert k.get(".group_segment_fixed_size", 0) == 0, want
        if "pre_kernel" in want:
            # a streaming kernel whose latency occupancy hides: 8 waves per SIMD
            assert k[".vgpr_count"] <= 64, (want, k[".vgpr_count"])
        else:
            # the look-ahead is two batches of 32 x 4 registers and must stay in
            # registers; addresses, accumulator and tail get 32 more at most
            assert 256 <= k[".vgpr_count"] <= 288, (want, k[".vgpr_count"])
        for (name, w, vn), ceiling in PARENT_VGPRS.items():
            if name == want and instance(want, w, vn) in k[".name"]:
                assert k[".vgpr_count"] <= ceiling, (want, w, vn, k[".vgpr_count"], ceiling)


def test_the_ragged_encode_kernel_still_has_its_twenty_instances(found):
    """The checksum is a run-time branch of one lane, not a template parameter.
    The ragged instantiations are those of encode_kernel whose tables argument
    is RaggedTabs (its ragged mode)."""
    meta = kernel_meta.kernels(LIB)
    assert len([n for n in meta if "encode_kernel" in n and "RaggedTabs" in n]) == 20
