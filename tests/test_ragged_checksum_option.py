"""CMP_GPU_OPT_IMAGE_RAGGED_CHECKSUM and airs_dev_ragged_ck_stats on the real
library with no GPU present.  The option is a host-side plan like options 4
and 5: cmp_gpu_engine_set_option stores it in the engine and never reaches the
device layer, so a placeholder engine (zeroed memory, a NULL device engine)
answers.  The counters follow the copy-and-return convention of
airs_dev_ragged_stats."""
import ctypes

import pytest

from conftest import load_pkg

pkg = load_pkg()
api = pkg.cmpapi


def set_option(prod):
    fn = prod.lib.cmp_gpu_engine_set_option
    fn.argtypes, fn.restype = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32], ctypes.c_uint32
    return fn


def test_the_option_has_its_number():
    assert pkg.OPT_IMAGE_RAGGED_CHECKSUM == 6 and api.GPU_OPT_IMAGE_RAGGED_CHECKSUM == 6


@pytest.mark.parametrize("value", [0, 1])
def test_set_option_accepts_the_value_on_the_host(prod, value):
    eng = ctypes.create_string_buffer(64)  # struct cmp_gpu_engine: dev NULL, the options 0
    fn = set_option(prod)
    assert fn(ctypes.addressof(eng), pkg.OPT_IMAGE_RAGGED_CHECKSUM, value) == 0
    assert fn(ctypes.addressof(eng), pkg.OPT_IMAGE_RAGGED, 1) == 0
    assert fn(ctypes.addressof(eng), pkg.OPT_IMAGE_CHUNK, 4096) == 0


@pytest.mark.parametrize("value", [2, 65536, 0xFFFFFFFF])
def test_set_option_refuses_any_other_value(prod, value):
    eng = ctypes.create_string_buffer(64)
    fn = set_option(prod)
    assert fn(ctypes.addressof(eng), pkg.OPT_IMAGE_RAGGED_CHECKSUM, 1) == 0
    before = eng.raw
    assert fn(ctypes.addressof(eng), pkg.OPT_IMAGE_RAGGED_CHECKSUM, value) == api.err_value("PARAMS_INVALID")
    assert eng.raw == before  # a refused value leaves the engine as it was


@pytest.mark.parametrize("value", [0, 1, 2])
def test_set_option_refuses_a_null_engine(prod, value):
    assert set_option(prod)(None, pkg.OPT_IMAGE_RAGGED_CHECKSUM, value) == api.err_value("GENERIC")


def test_ragged_ck_stats_copy_and_return(prod):
    fn = prod.lib.airs_dev_ragged_ck_stats
    fn.argtypes, fn.restype = [ctypes.c_void_p, ctypes.c_uint32], ctypes.c_uint32
    mark = 0xA5A5A5A5A5A5A5A5
    out = (ctypes.c_uint64 * 4)(*([mark] * 4))
    assert fn(out, 4) == 2  # launches, frames
    assert list(out)[2:] == [mark, mark]
    full = list(out)[:2]
    one = (ctypes.c_uint64 * 4)(*([mark] * 4))
    assert fn(one, 1) == 2
    assert list(one) == [full[0], mark, mark, mark]
    assert fn(None, 0) == 2


def test_the_ragged_counters_are_still_three(prod):
    fn = prod.lib.airs_dev_ragged_stats
    fn.argtypes, fn.restype = [ctypes.c_void_p, ctypes.c_uint32], ctypes.c_uint32
    assert fn(None, 0) == 3
