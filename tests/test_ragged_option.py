"""CMP_GPU_OPT_IMAGE_RAGGED and airs_dev_ragged_stats on the real library with
no GPU present.  The option is a host-side plan: cmp_gpu_engine_set_option
stores it in the engine and never reaches the device layer, so a placeholder
engine (zeroed memory, a NULL device engine) answers.  The counters follow the
copy-and-return convention of airs_dev_encode_image_stats."""
import ctypes

import pytest

from conftest import load_pkg

pkg = load_pkg()
api = pkg.cmpapi


def test_the_option_has_its_number():
    assert pkg.OPT_IMAGE_RAGGED == 5 and api.GPU_OPT_IMAGE_RAGGED == 5


@pytest.mark.parametrize("value", [0, 1, 65536])
def test_set_option_accepts_the_value_on_the_host(prod, value):
    eng = ctypes.create_string_buffer(64)  # struct cmp_gpu_engine: dev NULL, the options 0
    fn = prod.lib.cmp_gpu_engine_set_option
    fn.argtypes, fn.restype = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32], ctypes.c_uint32
    assert fn(ctypes.addressof(eng), pkg.OPT_IMAGE_RAGGED, value) == 0
    assert fn(ctypes.addressof(eng), pkg.OPT_IMAGE_CHUNK, 4096) == 0
    assert fn(None, pkg.OPT_IMAGE_RAGGED, value) == api.err_value("GENERIC")


def test_ragged_stats_copy_and_return(prod):
    fn = prod.lib.airs_dev_ragged_stats
    fn.argtypes, fn.restype = [ctypes.c_void_p, ctypes.c_uint32], ctypes.c_uint32
    mark = 0xA5A5A5A5A5A5A5A5
    out = (ctypes.c_uint64 * 5)(*([mark] * 5))
    assert fn(out, 5) == 3  # launches, frames, blocks
    assert list(out)[3:] == [mark, mark]
    full = list(out)[:3]
    one = (ctypes.c_uint64 * 5)(*([mark] * 5))
    assert fn(one, 1) == 3
    assert list(one) == [full[0], mark, mark, mark, mark]
    assert fn(None, 0) == 3
