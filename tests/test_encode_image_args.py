"""cmp_gpu_compress_image: the call-level refusals, in the order the header
documents.  Validation returns before anything touches the device, so the real
library answers them with no GPU present; the engine and the device pointers
are never dereferenced (placeholders).  The two host tables and the context
are read, so they are real."""
import ctypes

import numpy as np
import pytest

from conftest import load_pkg

pkg = load_pkg()
api = pkg.cmpapi

BASE = 1 << 20  # a 16-byte aligned placeholder address
OFFS = np.array([3, 1000, 17, 2000, 17], dtype=np.uint64)
SIZES = np.array([200, 64, 200, 96, 2], dtype=np.uint32)


def good():
    return dict(type=pkg.GPU_U16, src=BASE + 3, src_size=4096, offsets=OFFS.ctypes.data,
                frame_bytes=SIZES.ctypes.data, num_frames=5, out=3 * BASE + 5, out_capacity=1 << 20,
                out_offsets=4 * BASE, sizes=5 * BASE, batch_flags=api.GPU_AUTO_RICE,
                flags=pkg.IMG_SRC_BIG_ENDIAN)


def table(offs, sizes):
    o, s = np.array(offs, dtype=np.uint64), np.array(sizes, dtype=np.uint32)
    KEEP.extend((o, s))
    return dict(offsets=o.ctypes.data, frame_bytes=s.ctypes.data, num_frames=len(offs))


KEEP = []
BAD = {
    "offsets NULL": (dict(offsets=None), "GENERIC"),
    "frame_bytes NULL": (dict(frame_bytes=None), "GENERIC"),
    "out_offsets NULL": (dict(out_offsets=None), "GENERIC"),
    "sizes NULL": (dict(sizes=None), "GENERIC"),
    "no frames": (dict(num_frames=0), "GENERIC"),
    "src NULL": (dict(src=None), "SRC_NULL"),
    "src_size 0": (dict(src_size=0), "SRC_SIZE_WRONG"),
    "a frame past the end": (table([0, 4000], [64, 98]), "SRC_SIZE_WRONG"),
    "an offset past the end": (table([0, 4097], [64, 0]), "SRC_SIZE_WRONG"),
    "an offset that wraps": (table([0, 2 ** 64 - 2], [64, 4]), "SRC_SIZE_WRONG"),
    "out NULL": (dict(out=None), "DST_NULL"),
    "out_offsets misaligned": (dict(out_offsets=4 * BASE + 4), "GENERIC"),
    "sizes misaligned": (dict(sizes=5 * BASE + 2), "GENERIC"),
    "unknown sample type": (dict(type=3), "GENERIC"),
    "unknown flag": (dict(flags=0x2), "GENERIC"),
    "unknown batch flag": (dict(batch_flags=0x10), "GENERIC"),
    "REPORT_DRAWS": (dict(batch_flags=pkg.REPORT_DRAWS), "GENERIC"),
    "big-endian i16-in-i32": (dict(type=pkg.GPU_I16_IN_I32), "GENERIC"),
    # the order of the checks: the first one that applies
    "no frames before src NULL": (dict(num_frames=0, src=None), "GENERIC"),
    "src NULL before src_size 0": (dict(src=None, src_size=0), "SRC_NULL"),
    "src_size before out NULL": (dict(src_size=201, out=None), "SRC_SIZE_WRONG"),
    "out NULL before misaligned sizes": (dict(out=None, sizes=5 * BASE + 1), "DST_NULL"),
    "misaligned sizes before an unknown flag": (dict(sizes=5 * BASE + 1, flags=0x80), "GENERIC"),
}


def context(prod, valid=True):
    ctx = api.CmpContext()
    if valid:
        params = api.CmpParams(primary_preprocessing=1, primary_encoder_type=1, primary_encoder_param=32)
        assert not api.is_error(prod.initialise(ctx, params))
    return ctx


def call(prod, ctx, change, engine=True):
    eng = ctypes.create_string_buffer(64)  # never read: every case fails validation
    b = pkg.GpuEncodeImage(**dict(good(), **change))
    return api.error_name(prod.lib.cmp_gpu_compress_image(ctypes.addressof(eng) if engine else None,
                                                          ctypes.byref(ctx) if ctx is not None else None,
                                                          ctypes.byref(b)))


@pytest.mark.parametrize("what", sorted(BAD))
def test_refused_before_the_device(prod, what):
    change, want = BAD[what]
    assert call(prod, context(prod), change) == want, what


def test_the_table_edge_is_accepted_by_the_size_check(prod):
    """A frame that ends exactly at src_size passes the size check: the call
    goes on to the next refusal (here the context)."""
    assert call(prod, context(prod, valid=False), table([4096 - 64, 4096], [64, 0])) == "CONTEXT_INVALID"


def test_null_engine_context_and_image(prod):
    ctx = context(prod)
    assert call(prod, ctx, {}, engine=False) == "GENERIC"
    assert call(prod, None, {}) == "GENERIC"
    eng = ctypes.create_string_buffer(64)
    assert api.error_name(prod.lib.cmp_gpu_compress_image(ctypes.addressof(eng), ctypes.byref(ctx), None)) == "GENERIC"


def test_an_invalid_context_is_refused_last(prod):
    """As cmp_gpu_compress refuses it, after every refusal of the arguments."""
    ctx = context(prod, valid=False)
    assert call(prod, ctx, {}) == "CONTEXT_INVALID"
    assert call(prod, ctx, dict(type=pkg.GPU_I16_IN_I32)) == "GENERIC"
    assert call(prod, ctx, dict(out=None)) == "DST_NULL"
    # a context that keeps its model in the work buffer: an odd (device) pointer
    params = api.CmpParams(primary_preprocessing=1, primary_encoder_type=1, primary_encoder_param=32,
                           secondary_iterations=2, secondary_preprocessing=3, secondary_encoder_type=1,
                           secondary_encoder_param=8, model_rate=8)
    ctx = api.CmpContext()
    wb = api.aligned_empty(4096)
    assert not api.is_error(prod.initialise(ctx, params, wb, 4096))
    ctx.work_buf = ctx.work_buf + 1
    assert call(prod, ctx, {}) == "WORK_BUF_UNALIGNED"


def test_struct_matches_the_header():
    # include/cmp_gpu.h: struct cmp_gpu_encode_image on LP64
    f = pkg.GpuEncodeImage
    assert (f.src.offset, f.src_size.offset, f.offsets.offset, f.frame_bytes.offset) == (8, 16, 24, 32)
    assert (f.num_frames.offset, f.out.offset, f.out_capacity.offset, f.out_offsets.offset) == (40, 48, 56, 64)
    assert (f.sizes.offset, f.batch_flags.offset, f.flags.offset, ctypes.sizeof(f)) == (72, 80, 84, 88)
    assert pkg.IMG_SRC_BIG_ENDIAN == 1
