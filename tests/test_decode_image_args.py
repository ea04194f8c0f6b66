"""cmp_gpu_decompress_image: the call-level refusals that need no header.
Validation returns before anything touches the device, so the real library
answers them with no GPU present; the engine and the pointers are never
dereferenced (placeholders).  And cmp_gpu_frame_table, which is host code,
against a Python walk."""
import ctypes

import numpy as np
import pytest

import image_helpers as ih
from conftest import load_pkg

pkg = load_pkg()
api = pkg.cmpapi

BASE = 1 << 20  # a 16-byte aligned placeholder address


def good():
    return dict(type=pkg.GPU_U16, src=BASE + 3, src_size=4096, offsets=2 * BASE, num_frames=5, dst=3 * BASE + 2,
                dst_capacity=1 << 20, dst_offsets=4 * BASE, status=5 * BASE, checksum_ok=6 * BASE, model=7 * BASE + 2,
                model_samples=1024, model_n=8 * BASE, flags=pkg.IMG_MODEL_IN | pkg.IMG_BIG_ENDIAN)


BAD = {
    "offsets NULL": (dict(offsets=None), "GENERIC"),
    "dst_offsets NULL": (dict(dst_offsets=None), "GENERIC"),
    "status NULL": (dict(status=None), "GENERIC"),
    "no frames": (dict(num_frames=0), "GENERIC"),
    "src NULL": (dict(src=None), "SRC_NULL"),
    "src_size 0": (dict(src_size=0), "SRC_SIZE_WRONG"),
    "dst NULL": (dict(dst=None), "DST_NULL"),
    "dst odd": (dict(dst=3 * BASE + 1), "DST_UNALIGNED"),
    "unknown sample type": (dict(type=3), "GENERIC"),
    "unknown flag": (dict(flags=0x4), "GENERIC"),
    "model without model_n": (dict(model_n=None), "GENERIC"),
    "model odd": (dict(model=7 * BASE + 1), "GENERIC"),
    "model of no samples": (dict(model_samples=0), "GENERIC"),
    "MODEL_IN without model": (dict(model=None, model_n=None), "GENERIC"),
    # the order of the checks: the first one that applies
    "src NULL before dst NULL": (dict(src=None, dst=None), "SRC_NULL"),
    "no frames before src NULL": (dict(num_frames=0, src=None), "GENERIC"),
    "dst NULL before an unknown flag": (dict(dst=None, flags=0x80), "DST_NULL"),
}


@pytest.mark.parametrize("what", sorted(BAD))
def test_refused_before_the_device(prod, what):
    engine = ctypes.create_string_buffer(64)  # never read: every case fails validation
    change, want = BAD[what]
    b = pkg.GpuDecodeImage(**dict(good(), **change))
    r = prod.lib.cmp_gpu_decompress_image(ctypes.addressof(engine), ctypes.byref(b))
    assert api.error_name(r) == want, what


def test_null_engine_and_batch(prod):
    b = pkg.GpuDecodeImage(**good())
    assert api.error_name(prod.lib.cmp_gpu_decompress_image(None, ctypes.byref(b))) == "GENERIC"
    engine = ctypes.create_string_buffer(64)
    assert api.error_name(prod.lib.cmp_gpu_decompress_image(ctypes.addressof(engine), None)) == "GENERIC"


def test_struct_matches_the_header():
    # include/cmp_gpu.h: struct cmp_gpu_decode_image on LP64
    f = pkg.GpuDecodeImage
    assert (f.src.offset, f.src_size.offset, f.offsets.offset, f.num_frames.offset) == (8, 16, 24, 32)
    assert (f.dst.offset, f.dst_capacity.offset, f.dst_offsets.offset, f.status.offset) == (40, 48, 56, 64)
    assert (f.checksum_ok.offset, f.model.offset, f.model_samples.offset, f.model_n.offset) == (72, 80, 88, 96)
    assert (f.flags.offset, ctypes.sizeof(f)) == (104, 112)
    assert (pkg.IMG_MODEL_IN, pkg.IMG_BIG_ENDIAN, pkg.OPT_IMAGE_CHUNK) == (1, 2, 4)


def frame(size, fill=0):
    """`size` bytes that walk as one frame (only bytes 2..4 matter to the walk)."""
    b = bytearray([fill]) * size
    b[2:5] = size.to_bytes(3, "big")
    return bytes(b)


def images():
    rng = np.random.default_rng(4)
    good = b"".join(frame(int(s), 0xEE) for s in rng.integers(16, 300, 40))
    return {
        "good": good,
        "one frame": frame(16),
        "the largest frame": frame((1 << 24) - 1, 0xFF) + frame(16),
        "empty": b"",
        "truncated tail": good[:-7],
        "15 bytes left": good + bytes(15),
        "frame size 15": frame(20) + frame(15) + frame(30),
        "frame size 0": frame(20) + bytes(40),
        "first frame bad": bytes(16),
        "shorter than a header": bytes(5),
    }


IMAGES = images()


@pytest.mark.parametrize("what", sorted(IMAGES))
def test_frame_table_against_a_python_walk(prod, what):
    blob = IMAGES[what]
    want, bad = ih.walk(blob)
    count, offs, bad_at = prod.frame_table(blob)
    assert count == len(want) and [int(o) for o in offs] == want and bad_at == bad, what
    # fewer slots than frames: the count is the frames found, the slots hold the first ones
    room = len(want) // 2
    guard = np.full(room + 2, 2 ** 64 - 1, dtype=np.uint64)
    buf = np.frombuffer(blob, dtype=np.uint8)
    b = ctypes.c_uint64(7)
    n = prod.lib.cmp_gpu_frame_table(buf.ctypes.data if buf.size else None, buf.size, guard.ctypes.data, room,
                                     ctypes.byref(b))
    assert n == len(want) and [int(o) for o in guard[:room]] == want[:room]
    assert (guard[room:] == 2 ** 64 - 1).all(), "written past max_frames"
    assert b.value == (2 ** 64 - 1 if bad is None else bad)
    # offsets NULL and bad_at NULL: count only
    assert prod.lib.cmp_gpu_frame_table(buf.ctypes.data if buf.size else None, buf.size, None, 1 << 40, None) == n


def test_frame_table_expectations():
    """The Python walk itself, on cases whose answer is known by hand."""
    assert ih.walk(IMAGES["empty"]) == ([], None)
    assert ih.walk(IMAGES["frame size 15"]) == ([0], 20)
    assert ih.walk(IMAGES["15 bytes left"])[1] == len(IMAGES["good"])
    assert ih.walk(IMAGES["truncated tail"])[1] is not None
    assert ih.walk(IMAGES["good"])[1] is None and len(ih.walk(IMAGES["good"])[0]) == 40
