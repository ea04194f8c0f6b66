"""cmp_gpu_decompress_sequences: the call-level refusals.  Validation returns
before anything touches the device, so the real library answers them with no
GPU present; the engine and the pointers are never dereferenced (placeholders)."""
import ctypes

import pytest

from conftest import load_pkg

pkg = load_pkg()
api = pkg.cmpapi

BASE = 1 << 20  # a 16-byte aligned placeholder address


def good():
    return dict(type=pkg.GPU_U16, src=BASE, src_stride=4096, src_capacity=4096, num_ctx=3, frames_per_ctx=6,
                dst=2 * BASE, dst_stride=2048, dst_samples=1024, status=3 * BASE, model=4 * BASE, model_stride=2048,
                model_n=5 * BASE, checksum_ok=6 * BASE, flags=pkg.SEQ_MODEL_IN)


BAD = {
    "src NULL": dict(src=None),
    "dst NULL": dict(dst=None),
    "status NULL": dict(status=None),
    "no contexts": dict(num_ctx=0),
    "no frames": dict(frames_per_ctx=0),
    "src misaligned": dict(src=BASE + 4),
    "src_stride misaligned": dict(src_stride=4100),
    "src_stride below src_capacity": dict(src_stride=2048),
    "src_capacity below a header": dict(src_capacity=20),
    "src_capacity no multiple of 4": dict(src_capacity=4094),
    "dst odd": dict(dst=2 * BASE + 1),
    "dst_stride odd": dict(dst_stride=2049),
    "dst rows overlap": dict(dst_stride=2046),
    "65536 frames": dict(num_ctx=4096, frames_per_ctx=16),
    "frame count overflows 32 bits": dict(num_ctx=1 << 31, frames_per_ctx=2),
    "model without model_n": dict(model_n=None),
    "model odd": dict(model=4 * BASE + 1),
    "model_stride odd": dict(model_stride=2049),
    "model rows overlap": dict(model_stride=1024),
    "MODEL_IN without model": dict(model=None, model_n=None),
    "unknown flag": dict(flags=0x10),
    "unknown sample type": dict(type=3),
}


@pytest.mark.parametrize("what", sorted(BAD))
def test_refused_before_the_device(prod, what):
    engine = ctypes.create_string_buffer(64)  # never read: every case fails validation
    b = pkg.GpuDecodeSeqBatch(**dict(good(), **BAD[what]))
    r = prod.lib.cmp_gpu_decompress_sequences(ctypes.addressof(engine), ctypes.byref(b))
    assert api.error_name(r) == "GENERIC", what


def test_null_engine_and_batch(prod):
    b = pkg.GpuDecodeSeqBatch(**good())
    assert api.error_name(prod.lib.cmp_gpu_decompress_sequences(None, ctypes.byref(b))) == "GENERIC"
    engine = ctypes.create_string_buffer(64)
    assert api.error_name(prod.lib.cmp_gpu_decompress_sequences(ctypes.addressof(engine), None)) == "GENERIC"


def test_struct_matches_the_header():
    # include/cmp_gpu.h: struct cmp_gpu_decode_seq_batch on LP64
    f = pkg.GpuDecodeSeqBatch
    assert (f.src.offset, f.src_capacity.offset, f.num_ctx.offset, f.frames_per_ctx.offset) == (8, 24, 28, 32)
    assert (f.dst.offset, f.dst_samples.offset, f.status.offset, f.model.offset) == (40, 56, 64, 72)
    assert (f.model_n.offset, f.checksum_ok.offset, f.flags.offset, ctypes.sizeof(f)) == (88, 96, 104, 112)
