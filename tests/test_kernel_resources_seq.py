"""The decoder's chain kernel (dec_seq_chain_kernel, decode.hip) in the built
library's code-object metadata (tests/kernel_meta.py; no GPU): both forms are
there, without VGPR spills or scratch.  It is a streaming kernel whose latency
is hidden by occupancy: at most 64 VGPRs (8 waves per SIMD)."""
import os

import pytest

import kernel_meta
from conftest import PKG_DIR

LIB = os.path.join(PKG_DIR, "lib", "libairscmp.so")


@pytest.fixture(scope="module")
def chain(prod):
    meta = kernel_meta.kernels(LIB)
    return {n: k for n, k in meta.items() if "dec_seq_chain_kernel" in n}


def test_chain_kernel_is_in_the_library(chain):
    # the zero-extending (u16) and the sign-extending form
    assert sorted("ILb1E" in n for n in chain) == [False, True], sorted(chain)


def test_chain_kernel_has_no_spills_or_scratch(chain):
    assert chain
    for n, k in chain.items():
        assert k[".vgpr_spill_count"] == 0, (n, k[".vgpr_spill_count"])
        assert k[".sgpr_spill_count"] == 0, (n, k[".sgpr_spill_count"])
        assert k.get(".private_segment_fixed_size", 0) == 0, n
        assert k[".vgpr_count"] <= 64, (n, k[".vgpr_count"])
