"""airs-compression_amd -- MI355X-native AIRSPACE encode path.

Python side of the drop-in: ctypes bindings over ``lib/libairscmp.so``
(built from ``csrc/`` by the Makefile).  ``cmpapi`` mirrors the reference's
lib/cmp.h API; :class:`GpuEngine` binds the device batch API of
include/cmp_gpu.h.  The library has no CPU encode path: compress calls need
the HIP device, and loading fails loudly when the shared object is missing.
"""
from __future__ import annotations

import ctypes
import os
import subprocess
from ctypes import POINTER, c_int, c_uint32, c_uint64, c_void_p

from .cmpapi import *  # noqa: F401,F403
from .cmpapi import CmpContext, CmpLib, is_error, error_name

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(PKG_DIR, "lib", "libairscmp.so")

GPU_U16, GPU_I16, GPU_I16_IN_I32 = 0, 1, 2
GPU_AUTO_RICE = 0x1
REPORT_DRAWS = 0x8  # CMP_GPU_REPORT_DRAWS
SEQ_MODEL_IN = 0x1  # CMP_GPU_SEQ_MODEL_IN (cmp_gpu_decompress_sequences)
STREAM_DECODE_MAX = 536870400  # CMP_GPU_STREAM_DECODE_MAX: bytes cmp_gpu_decode_stream accepts (2^32 - 4096 bits)
LAYOUT_ROUNDROBIN, LAYOUT_BLOCK, LAYOUT_STREAMS = 0, 1, 2  # enum cmp_gpu_layout
GATHER_PATCH_IDS = 0x1  # CMP_GPU_GATHER_PATCH_IDS
OPT_EXCLUSIVE = 1  # cmp_gpu_engine_set_option (include/cmp_gpu.h)
OPT_WALK_SEGMENT = 2
OPT_NO_CONTEXT_WALK = 3
OPT_IMAGE_CHUNK = 4  # CMP_GPU_OPT_IMAGE_CHUNK: bytes of staging per chunk of decompress_image (0: 256 MiB)
# CMP_GPU_OPT_IMAGE_RAGGED: compress_image encodes frames of unequal sizes in one launch (0: off, 1: on,
# any other value: on with that keep threshold in bytes)
OPT_IMAGE_RAGGED = 5
# CMP_GPU_OPT_IMAGE_RAGGED_CHECKSUM: 1 lets checksum-enabled contexts take those launches too (0: off)
OPT_IMAGE_RAGGED_CHECKSUM = 6
IMG_MODEL_IN = 0x1  # CMP_GPU_IMG_MODEL_IN (cmp_gpu_decompress_image)
IMG_BIG_ENDIAN = 0x2  # CMP_GPU_IMG_BIG_ENDIAN
IMG_SRC_BIG_ENDIAN = 0x1  # CMP_GPU_IMG_SRC_BIG_ENDIAN (cmp_gpu_compress_image)
ESTIMATE_MAX_CANDIDATES = 64  # CMP_GPU_ESTIMATE_MAX_CANDIDATES
ESTIMATE_MAX_FRAMES = 1 << 20  # CMP_GPU_ESTIMATE_MAX_FRAMES
KIND_TO_GPU = {"u16": GPU_U16, "i16": GPU_I16, "i16_in_i32": GPU_I16_IN_I32}


def build(jobs: int = 8) -> str:
    """Compile csrc/ into lib/libairscmp.so (hipcc for gfx950 + gcc)."""
    subprocess.run(["make", f"-j{jobs}", "-C", PKG_DIR], check=True)
    return LIB_PATH


def _one_hip_runtime() -> None:
    """PyTorch-ROCm ships its own libamdhip64.so (SONAME libamdhip64.so.7, the
    same as /opt/rocm's).  If libairscmp.so were dlopen'ed first, torch would
    later map a second HIP runtime into the process and fail to see the GPU.
    Importing torch first makes the library bind to torch's copy, so device
    pointers, streams and events are shared.  Without torch the library uses
    /opt/rocm's runtime as usual."""
    try:
        import torch  # noqa: F401
    except ImportError:
        pass


def load(path: str | None = None) -> "AirsLib":
    # AIRS_LIB: developer override (benchmarking an alternative build)
    path = path or os.environ.get("AIRS_LIB") or LIB_PATH
    _one_hip_runtime()
    if not os.path.exists(path):
        raise FileNotFoundError(
            f"{path} is missing: build it with `make -C {PKG_DIR}` (no CPU fallback exists)")
    return AirsLib(path)


class GpuBatch(ctypes.Structure):
    """struct cmp_gpu_batch (include/cmp_gpu.h)."""
    _fields_ = [
        ("type", c_int),
        ("src", c_void_p),
        ("src_stride", c_uint64),
        ("src_size", c_uint32),
        ("dst", c_void_p),
        ("dst_stride", c_uint64),
        ("dst_capacity", c_uint32),
        ("sizes", c_void_p),
        ("flags", c_uint32),
        ("draws", c_void_p),
    ]


class GpuDecodeBatch(ctypes.Structure):
    """struct cmp_gpu_decode_batch (include/cmp_gpu.h)."""
    _fields_ = [
        ("src", c_void_p),
        ("src_stride", c_uint64),
        ("src_capacity", c_uint32),
        ("num_frames", c_uint32),
        ("dst", c_void_p),
        ("dst_stride", c_uint64),
        ("dst_samples", c_uint32),
        ("status", c_void_p),
        ("model", c_void_p),
        ("model_stride", c_uint64),
    ]


class GpuDecodeSeqBatch(ctypes.Structure):
    """struct cmp_gpu_decode_seq_batch (include/cmp_gpu.h)."""
    _fields_ = [
        ("type", c_int),
        ("src", c_void_p),
        ("src_stride", c_uint64),
        ("src_capacity", c_uint32),
        ("num_ctx", c_uint32),
        ("frames_per_ctx", c_uint32),
        ("dst", c_void_p),
        ("dst_stride", c_uint64),
        ("dst_samples", c_uint32),
        ("status", c_void_p),
        ("model", c_void_p),
        ("model_stride", c_uint64),
        ("model_n", c_void_p),
        ("checksum_ok", c_void_p),
        ("flags", c_uint32),
    ]


class GpuDecodeImage(ctypes.Structure):
    """struct cmp_gpu_decode_image (include/cmp_gpu.h)."""
    _fields_ = [
        ("type", c_int),
        ("src", c_void_p),
        ("src_size", c_uint64),
        ("offsets", c_void_p),
        ("num_frames", c_uint32),
        ("dst", c_void_p),
        ("dst_capacity", c_uint64),
        ("dst_offsets", c_void_p),
        ("status", c_void_p),
        ("checksum_ok", c_void_p),
        ("model", c_void_p),
        ("model_samples", c_uint32),
        ("model_n", c_void_p),
        ("flags", c_uint32),
    ]


class GpuEncodeImage(ctypes.Structure):
    """struct cmp_gpu_encode_image (include/cmp_gpu.h)."""
    _fields_ = [
        ("type", c_int),
        ("src", c_void_p),
        ("src_size", c_uint64),
        ("offsets", c_void_p),
        ("frame_bytes", c_void_p),
        ("num_frames", c_uint32),
        ("out", c_void_p),
        ("out_capacity", c_uint64),
        ("out_offsets", c_void_p),
        ("sizes", c_void_p),
        ("batch_flags", c_uint32),
        ("flags", c_uint32),
    ]


class GpuCandidate(ctypes.Structure):
    """struct cmp_gpu_candidate (include/cmp_gpu.h): one pass's parameters."""
    _fields_ = [
        ("preprocessing", c_int),
        ("encoder_type", c_int),
        ("encoder_param", c_uint32),
        ("encoder_outlier", c_uint32),
    ]


class GpuEstimateBatch(ctypes.Structure):
    """struct cmp_gpu_estimate_batch (include/cmp_gpu.h)."""
    _fields_ = [
        ("type", c_int),
        ("src", c_void_p),
        ("src_stride", c_uint64),
        ("src_size", c_uint32),
        ("num_frames", c_uint32),
        ("model", c_void_p),
        ("model_stride", c_uint64),
        ("candidates", POINTER(GpuCandidate)),
        ("num_candidates", c_uint32),
        ("bits", c_void_p),
        ("best", c_void_p),
        ("flags", c_uint32),
    ]


def candidate_array(candidates):
    """A ctypes GpuCandidate array from GpuCandidate objects or (preprocessing,
    encoder_type, encoder_param[, encoder_outlier]) tuples."""
    arr = (GpuCandidate * max(len(candidates), 1))()
    for i, c in enumerate(candidates):
        if isinstance(c, GpuCandidate):
            c = (c.preprocessing, c.encoder_type, c.encoder_param, c.encoder_outlier)
        arr[i] = GpuCandidate(*c)
    return arr


class AirsLib(CmpLib):
    """CmpLib plus the cmp_gpu.h device batch API."""

    def __init__(self, path: str = LIB_PATH):
        super().__init__(path)
        L = self.lib
        L.cmp_gpu_available.restype = c_int
        L.cmp_gpu_engine_create.argtypes = [POINTER(c_void_p), c_void_p]
        L.cmp_gpu_engine_create.restype = c_uint32
        L.cmp_gpu_engine_destroy.argtypes = [c_void_p]
        L.cmp_gpu_engine_destroy.restype = None
        L.cmp_gpu_engine_set_option.argtypes = [c_void_p, c_uint32, c_uint32]
        L.cmp_gpu_engine_set_option.restype = c_uint32
        L.cmp_gpu_compress.argtypes = [c_void_p, POINTER(CmpContext), c_uint32, c_uint32, POINTER(GpuBatch)]
        L.cmp_gpu_compress.restype = c_uint32
        L.cmp_gpu_synchronize.argtypes = [c_void_p]
        L.cmp_gpu_synchronize.restype = c_uint32
        L.cmp_gpu_synthesize.argtypes = [c_void_p, c_void_p, c_uint32, c_uint64, c_uint32, c_uint32,
                                         c_uint32, c_uint64, c_uint32]
        L.cmp_gpu_synthesize.restype = c_uint32
        L.cmp_gpu_decompress.argtypes = [c_void_p, POINTER(GpuDecodeBatch)]
        L.cmp_gpu_decompress.restype = c_uint32
        L.cmp_gpu_decompress_sequences.argtypes = [c_void_p, POINTER(GpuDecodeSeqBatch)]
        L.cmp_gpu_decompress_sequences.restype = c_uint32
        L.cmp_gpu_encode_stream.argtypes = [c_void_p, c_uint32, c_void_p, c_uint32, c_uint32, c_uint32, c_uint32,
                                            c_uint32, c_void_p, c_uint32, c_void_p]
        L.cmp_gpu_encode_stream.restype = c_uint32
        L.cmp_gpu_decode_stream.argtypes = [c_void_p, c_void_p, c_uint32, c_uint32, c_uint32, c_uint32, c_uint32,
                                            c_uint32, c_void_p, c_void_p]
        L.cmp_gpu_decode_stream.restype = c_uint32
        L.cmp_gpu_pack_frames.argtypes = [c_void_p, c_void_p, c_uint64, c_uint32, c_void_p, c_uint32, c_void_p,
                                          c_void_p]
        L.cmp_gpu_pack_frames.restype = c_uint32
        L.cmp_gpu_gather.argtypes = [c_void_p, c_void_p, c_uint32, c_uint32, c_uint32, c_void_p, c_uint64, c_uint32,
                                     c_void_p, c_void_p, c_uint32, c_void_p, c_uint64, c_void_p, c_void_p, c_uint64,
                                     c_uint32]
        L.cmp_gpu_gather.restype = c_uint32
        L.cmp_gpu_gather_plan.argtypes = [c_void_p, c_uint32, c_uint32, c_uint32, c_uint32, c_uint64, c_void_p,
                                          c_void_p, c_void_p, c_void_p]
        L.cmp_gpu_gather_plan.restype = c_uint32
        L.cmp_gpu_decompress_image.argtypes = [c_void_p, POINTER(GpuDecodeImage)]
        L.cmp_gpu_decompress_image.restype = c_uint32
        L.cmp_gpu_compress_image.argtypes = [c_void_p, POINTER(CmpContext), POINTER(GpuEncodeImage)]
        L.cmp_gpu_compress_image.restype = c_uint32
        L.cmp_gpu_frame_table.argtypes = [c_void_p, c_uint64, c_void_p, c_uint64, POINTER(c_uint64)]
        L.cmp_gpu_frame_table.restype = c_uint64
        L.cmp_gpu_estimate.argtypes = [c_void_p, POINTER(GpuEstimateBatch)]
        L.cmp_gpu_estimate.restype = c_uint32
        L.cmp_gpu_estimate_frame_size.argtypes = [POINTER(GpuCandidate), c_uint64, c_int]
        L.cmp_gpu_estimate_frame_size.restype = c_uint32

    def gpu_available(self) -> bool:
        return bool(self.lib.cmp_gpu_available())

    def gather_plan(self, entries, world: int, frames_per_rank: int, layout: int, fpc: int = 1,
                    id_base: int = 0, want_ids: bool = True):
        """cmp_gpu_gather_plan on host arrays (no device): entries uint64
        [world * frames_per_rank] = size | draws << 32.  Returns (rc,
        rank_bytes, offsets, sizes, ids or None), the last three in global
        frame order; ids UINT64_MAX where a frame keeps its identifier."""
        import numpy as np
        e = np.ascontiguousarray(entries, dtype=np.uint64)
        n = world * frames_per_rank
        rb = np.zeros(world, dtype=np.uint64)
        offs = np.zeros(max(n, 1), dtype=np.uint64)
        sz = np.zeros(max(n, 1), dtype=np.uint32)
        ids = np.zeros(max(n, 1), dtype=np.uint64) if want_ids else None
        r = self.lib.cmp_gpu_gather_plan(e.ctypes.data, world, frames_per_rank, layout, fpc, id_base, rb.ctypes.data,
                                         offs.ctypes.data, sz.ctypes.data, ids.ctypes.data if want_ids else None)
        return int(r), rb, offs[:n], sz[:n], (ids[:n] if want_ids else None)

    def frame_table(self, image, max_frames: int | None = None):
        """cmp_gpu_frame_table on a host image (bytes-like) of back-to-back frames
        (no device).  Returns (count, offsets, bad_at): the frames found, the
        uint64 offsets written (all of them, or the first max_frames) and the
        byte where the walk stopped short, or None when the image ends at a
        frame's end."""
        import numpy as np
        img = np.frombuffer(image, dtype=np.uint8)
        bad = c_uint64(0)
        ptr = img.ctypes.data if img.size else None
        count = int(self.lib.cmp_gpu_frame_table(ptr, img.size, None, 0, ctypes.byref(bad)))
        room = count if max_frames is None else max_frames
        offs = np.zeros(max(room, 1), dtype=np.uint64)
        self.lib.cmp_gpu_frame_table(ptr, img.size, offs.ctypes.data, room, ctypes.byref(bad))
        return count, offs[:min(room, count)], (None if bad.value == 2 ** 64 - 1 else int(bad.value))

    def estimate_frame_size(self, candidate, bits: int, checksum_enabled) -> int:
        """cmp_gpu_estimate_frame_size (no device): the size of the frame that holds
        `bits` payload bits coded with `candidate` (a GpuCandidate or a tuple, see
        candidate_array), or an error value."""
        c = None if candidate is None else candidate_array([candidate])
        return int(self.lib.cmp_gpu_estimate_frame_size(c, bits, 1 if checksum_enabled else 0))

    def engine(self, stream: int | None = None) -> "GpuEngine":
        return GpuEngine(self, stream)


class GpuEngine:
    """One cmp_gpu_engine bound to a HIP stream (raw hipStream_t handle)."""

    def __init__(self, lib: AirsLib, stream: int | None = None):
        self.lib = lib
        self.stream = stream  # raw hipStream_t the engine's work is queued on (None: the null stream)
        h = c_void_p()
        r = lib.lib.cmp_gpu_engine_create(ctypes.byref(h), stream)
        if is_error(r):
            raise RuntimeError(f"cmp_gpu_engine_create failed: {error_name(r)}")
        self.handle = h

    def set_option(self, option: int, value: int) -> int:
        """cmp_gpu_engine_set_option (OPT_EXCLUSIVE, OPT_WALK_SEGMENT, OPT_NO_CONTEXT_WALK, OPT_IMAGE_CHUNK,
        OPT_IMAGE_RAGGED, OPT_IMAGE_RAGGED_CHECKSUM)."""
        return int(self.lib.lib.cmp_gpu_engine_set_option(self.handle, option, value))

    def close(self):
        if self.handle:
            self.lib.lib.cmp_gpu_engine_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def compress(self, ctxs, frames_per_ctx: int, kind: str, src_ptr: int, src_stride: int,
                 src_size: int, dst_ptr: int, dst_stride: int, dst_capacity: int, sizes_ptr: int,
                 flags: int = 0, draws_ptr: int | None = None) -> int:
        """cmp_gpu_compress over device pointers; ctxs is a ctypes CmpContext array.
        draws_ptr: optional host uint8 array receiving each frame's identifier draws."""
        if draws_ptr:
            flags |= REPORT_DRAWS
        b = GpuBatch(type=KIND_TO_GPU[kind], src=src_ptr, src_stride=src_stride, src_size=src_size,
                     dst=dst_ptr, dst_stride=dst_stride, dst_capacity=dst_capacity,
                     sizes=sizes_ptr, flags=flags, draws=draws_ptr)
        n_ctx = len(ctxs)
        return self.lib.lib.cmp_gpu_compress(self.handle, ctxs, n_ctx, frames_per_ctx, ctypes.byref(b))

    def decompress(self, src_ptr: int, src_stride: int, src_capacity: int, num_frames: int, dst_ptr: int,
                   dst_stride: int, dst_samples: int, status_ptr: int, model_ptr: int = 0,
                   model_stride: int = 0) -> int:
        """cmp_gpu_decompress over device pointers (frames -> 16-bit samples)."""
        b = GpuDecodeBatch(src=src_ptr, src_stride=src_stride, src_capacity=src_capacity, num_frames=num_frames,
                           dst=dst_ptr, dst_stride=dst_stride, dst_samples=dst_samples, status=status_ptr,
                           model=model_ptr or None, model_stride=model_stride)
        return self.lib.lib.cmp_gpu_decompress(self.handle, ctypes.byref(b))

    def decompress_sequences(self, kind: str, src_ptr: int, src_stride: int, src_capacity: int, num_ctx: int,
                             frames_per_ctx: int, dst_ptr: int, dst_stride: int, dst_samples: int,
                             status_ptr: int, model_ptr: int = 0, model_stride: int = 0, model_n_ptr: int = 0,
                             checksum_ok_ptr: int = 0, flags: int = 0) -> int:
        """cmp_gpu_decompress_sequences over device pointers: num_ctx sequences of
        frames_per_ctx frames, MODEL frames decoded against the model rebuilt
        from the frames before them (flags: SEQ_MODEL_IN)."""
        b = GpuDecodeSeqBatch(type=KIND_TO_GPU[kind], src=src_ptr or None, src_stride=src_stride,
                              src_capacity=src_capacity, num_ctx=num_ctx, frames_per_ctx=frames_per_ctx,
                              dst=dst_ptr or None, dst_stride=dst_stride, dst_samples=dst_samples,
                              status=status_ptr or None, model=model_ptr or None, model_stride=model_stride,
                              model_n=model_n_ptr or None, checksum_ok=checksum_ok_ptr or None, flags=flags)
        return self.lib.lib.cmp_gpu_decompress_sequences(self.handle, ctypes.byref(b))

    def decompress_image(self, kind: str, src_ptr: int, src_size: int, offsets, dst_ptr: int, dst_capacity: int,
                         status_ptr: int, checksum_ok_ptr: int = 0, model_ptr: int = 0, model_samples: int = 0,
                         model_n_ptr: int = 0, flags: int = 0):
        """cmp_gpu_decompress_image: the frames at src + offsets[f] (host table,
        any alignment) decoded as one context into samples packed back to back
        at dst (flags: IMG_MODEL_IN, IMG_BIG_ENDIAN).  Returns (rc, dst_offsets):
        the host uint64 array [num_frames + 1] of each frame's byte offset in dst."""
        import numpy as np
        offs = np.ascontiguousarray(offsets, dtype=np.uint64)
        dof = np.zeros(offs.size + 1, dtype=np.uint64)
        b = GpuDecodeImage(type=KIND_TO_GPU[kind], src=src_ptr or None, src_size=src_size,
                           offsets=offs.ctypes.data, num_frames=offs.size, dst=dst_ptr or None,
                           dst_capacity=dst_capacity, dst_offsets=dof.ctypes.data, status=status_ptr or None,
                           checksum_ok=checksum_ok_ptr or None, model=model_ptr or None,
                           model_samples=model_samples, model_n=model_n_ptr or None, flags=flags)
        r = self.lib.lib.cmp_gpu_decompress_image(self.handle, ctypes.byref(b))
        return int(r), dof

    def compress_image(self, ctx, kind: str, src_ptr: int, src_size: int, offsets, frame_bytes, out_ptr: int,
                       out_capacity: int, out_offsets_ptr: int, sizes_ptr: int, batch_flags: int = 0,
                       flags: int = 0) -> int:
        """cmp_gpu_compress_image: the sample frames at src + offsets[f] (host
        tables of byte offsets and sizes, any alignment, unequal sizes)
        compressed as the ONE context ctx (a CmpContext) into a packed .air
        image at out; out_offsets (device uint64 [num_frames + 1]) and sizes
        (device uint32 [num_frames]) are valid after synchronize (flags:
        IMG_SRC_BIG_ENDIAN; batch_flags: GPU_AUTO_RICE, ...)."""
        import numpy as np
        offs = np.ascontiguousarray(offsets, dtype=np.uint64)
        fb = np.ascontiguousarray(frame_bytes, dtype=np.uint32)
        if offs.size != fb.size:
            raise ValueError("offsets and frame_bytes differ in length")
        b = GpuEncodeImage(type=KIND_TO_GPU[kind], src=src_ptr or None, src_size=src_size,
                           offsets=offs.ctypes.data, frame_bytes=fb.ctypes.data, num_frames=offs.size,
                           out=out_ptr or None, out_capacity=out_capacity, out_offsets=out_offsets_ptr or None,
                           sizes=sizes_ptr or None, batch_flags=batch_flags, flags=flags)
        return int(self.lib.lib.cmp_gpu_compress_image(self.handle, ctypes.byref(ctx), ctypes.byref(b)))

    def encode_stream(self, kind: str, src_ptr: int, num_samples: int, preprocessing: int, encoder_type: int,
                      encoder_param: int, encoder_outlier: int, dst_ptr: int, dst_capacity: int,
                      size_ptr: int) -> int:
        """cmp_gpu_encode_stream: one payload-only bit stream (no header) over device pointers."""
        return self.lib.lib.cmp_gpu_encode_stream(self.handle, KIND_TO_GPU[kind], src_ptr, num_samples,
                                                  preprocessing, encoder_type, encoder_param, encoder_outlier,
                                                  dst_ptr, dst_capacity, size_ptr)

    def decode_stream(self, src_ptr: int, src_size: int, num_samples: int, preprocessing: int, encoder_type: int,
                      encoder_param: int, encoder_outlier: int, dst_ptr: int, status_ptr: int) -> int:
        """cmp_gpu_decode_stream: the inverse of encode_stream over device pointers (src_size bytes of
        stream -> num_samples 16-bit samples; *status: num_samples or an error value after synchronize)."""
        return self.lib.lib.cmp_gpu_decode_stream(self.handle, src_ptr or None, src_size, num_samples, preprocessing,
                                                  encoder_type, encoder_param, encoder_outlier, dst_ptr or None,
                                                  status_ptr or None)

    def estimate(self, kind: str, src_ptr: int, src_stride: int, src_size: int, num_frames: int, candidates,
                 bits_ptr: int, best_ptr: int = 0, model_ptr: int = 0, model_stride: int = 0) -> int:
        """cmp_gpu_estimate over device pointers: bits[f * len(candidates) + c]
        (uint64) = the payload bits of frame f under candidate c, best[f]
        (uint32, optional) = the candidate of the smallest frame; both valid
        after synchronize.  candidates: GpuCandidate objects or tuples (see
        candidate_array)."""
        arr = candidates if isinstance(candidates, ctypes.Array) else candidate_array(candidates)
        b = GpuEstimateBatch(type=KIND_TO_GPU[kind], src=src_ptr or None, src_stride=src_stride, src_size=src_size,
                             num_frames=num_frames, model=model_ptr or None, model_stride=model_stride,
                             candidates=arr, num_candidates=len(candidates), bits=bits_ptr or None,
                             best=best_ptr or None, flags=0)
        return int(self.lib.lib.cmp_gpu_estimate(self.handle, ctypes.byref(b)))

    def pack_frames(self, frames_ptr: int, frame_stride: int, frame_capacity: int, sizes_ptr: int,
                    num_frames: int, out_ptr: int, offsets_ptr: int) -> int:
        """cmp_gpu_pack_frames: strided frames -> back to back at 8-byte aligned offsets (device)."""
        return self.lib.lib.cmp_gpu_pack_frames(self.handle, frames_ptr, frame_stride, frame_capacity, sizes_ptr,
                                                num_frames, out_ptr, offsets_ptr)

    def gather(self, nccl_comm: int, root: int, layout: int, fpc: int, frames_ptr: int, frame_stride: int,
               frame_capacity: int, sizes_ptr: int, draws_ptr: int | None, frames_per_rank: int, out_ptr: int | None,
               out_capacity: int, offsets_ptr: int | None, out_sizes_ptr: int | None, id_base: int = 0,
               flags: int = 0) -> int:
        """cmp_gpu_gather: every rank's frames on `root` over an RCCL communicator (ncclComm_t as an int)."""
        return self.lib.lib.cmp_gpu_gather(self.handle, nccl_comm, root, layout, fpc, frames_ptr, frame_stride,
                                           frame_capacity, sizes_ptr, draws_ptr, frames_per_rank, out_ptr,
                                           out_capacity, offsets_ptr, out_sizes_ptr, id_base, flags)

    def synchronize(self) -> int:
        return self.lib.lib.cmp_gpu_synchronize(self.handle)

    def synthesize(self, dst_ptr: int, sample_bytes: int, seed: int, frame0: int, n: int,
                   num_frames: int, stride: int, noise_w: int) -> int:
        return self.lib.lib.cmp_gpu_synthesize(self.handle, dst_ptr, sample_bytes, seed, frame0, n,
                                               num_frames, stride, noise_w)


def context_array(n: int):
    return (CmpContext * n)()


def __getattr__(name):
    # submodules that need torch are imported on first use
    if name == "shard":
        import importlib
        return importlib.import_module(__name__ + ".shard")
    raise AttributeError(name)
