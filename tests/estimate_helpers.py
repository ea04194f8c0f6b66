"""Shared pieces of the estimator's tests (test_gpu_estimate.py,
test_estimate_frame_size.py): sample generators, the oracle's exact payload
bits and the GPU runner with its guard words.

The exact bits come from the oracle by an identity: the NONE stream of a
residual sequence tiled 8 times has exactly as many bytes as the sequence's
payload has bits (8 copies of b bits are 8 b bits = b bytes, and the flush adds
nothing to whole bytes)."""
import ctypes

import numpy as np

import streams
from conftest import load_pkg

pkg = load_pkg()
api = pkg.cmpapi

NONE, DIFF, IWT, MODEL = api.PREPROCESS_NONE, api.PREPROCESS_DIFF, api.PREPROCESS_IWT, api.PREPROCESS_MODEL
RAW, ZERO, MULTI = api.ENCODER_UNCOMPRESSED, api.ENCODER_GOLOMB_ZERO, api.ENCODER_GOLOMB_MULTI
EST_SIZE, EST_FINISH, EST_IWT = range(3)  # airs_dev.h enum airs_est_stat
GUARD = 8      # guard words on either side of bits and best


def header_bytes(c):
    return 16 if c[0] == NONE and c[1] == RAW else 22


def low16(rng, n, walk=None):
    """n 16-bit patterns (uint16): Laplace noise, or its random walk."""
    v = rng.laplace(0, 2.0 ** rng.uniform(0, 13), n)
    if rng.random() < 0.5 if walk is None else walk:
        v = np.cumsum(v) * 0.05
    return (np.clip(np.round(v), -32768, 32767).astype(np.int64) & 0xFFFF).astype(np.uint16)


def as_kind(rng, lo, kind):
    """The patterns as a frame of the sample type; i16_in_i32 gets junk upper halves."""
    if kind == "u16":
        return lo.copy()
    if kind == "i16":
        return lo.view(np.int16).copy()
    hi = rng.integers(-30000, 30000, lo.size).astype(np.int64) << 16
    return (lo.astype(np.int64) | hi).astype(np.int32)


def residuals(lo, pre, model=None):
    """The 16-bit residuals (int16) the coder sees: one numpy subtraction."""
    x = lo.astype(np.int64)
    if pre == DIFF:
        x = x - np.concatenate(([0], x[:-1]))
    elif pre == MODEL:
        x = x - model.astype(np.int64)
    return (x & 0xFFFF).astype(np.uint16).view(np.int16)


def exact_bits(res, enc, g, outl):
    """The payload bits of the residuals: the byte count of the oracle's NONE
    stream over them tiled 8 times."""
    r, _ = streams.oracle_stream(np.tile(res, 8), "i16", NONE, enc, g, outl)
    assert not api.is_error(r), api.error_name(r)
    return r


def estimate_stats(prod):
    """The estimator's process-wide launch counters (airs_dev_estimate_stats):
    [sizing launches, finishing launches, IWT transforms]."""
    fn = prod.lib.airs_dev_estimate_stats
    fn.argtypes = [ctypes.POINTER(ctypes.c_uint64), ctypes.c_uint32]
    fn.restype = ctypes.c_uint32
    out = (ctypes.c_uint64 * 3)()
    assert fn(out, 3) == 3
    return [int(v) for v in out]


def run(eng, kind, frames, cands, pad=48, offset=0, want_best=True, models=None, model_pad=6, model_offset=0):
    """One cmp_gpu_estimate call over the frames (equal sizes): frame f at a
    stride of its size rounded up to 16 plus `pad` bytes, `offset` bytes past a
    16-byte boundary, poison everywhere else; models likewise.  bits and best
    lie between guard words, which must keep their values.  Returns (bits
    [frames, candidates] as Python ints in a uint64 array, best or None)."""
    import torch
    nf, nc = len(frames), len(cands)
    sb = frames[0].itemsize
    size = frames[0].size * sb
    stride = (size + 15) // 16 * 16 + pad
    host = np.full(16 + offset + nf * stride, 0xA5, dtype=np.uint8)
    for f, x in enumerate(frames):
        host[16 + offset + f * stride:16 + offset + f * stride + size] = np.ascontiguousarray(x).view(np.uint8)
    src = torch.from_numpy(host).cuda()
    mptr = mstride = 0
    if models is not None:
        msize = 2 * models[0].size
        mstride = (msize + 15) // 16 * 16 + model_pad
        mh = np.full(16 + model_offset + nf * mstride, 0x5A, dtype=np.uint8)
        for f, m in enumerate(models):
            mh[16 + model_offset + f * mstride:16 + model_offset + f * mstride + msize] = m.view(np.uint8)
        mdev = torch.from_numpy(mh).cuda()
        mptr = mdev.data_ptr() + 16 + model_offset
    gb, gw = 0x5151515151515151, 0x71717171
    bits = torch.full((nf * nc + 2 * GUARD,), gb, dtype=torch.int64, device="cuda")
    best = torch.full((nf + 2 * GUARD,), gw, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    r = eng.estimate(kind, src.data_ptr() + 16 + offset, stride, size, nf, cands, bits.data_ptr() + 8 * GUARD,
                     best.data_ptr() + 4 * GUARD if want_best else 0, mptr, mstride)
    assert r == 0, api.error_name(r)
    assert eng.synchronize() == 0
    b, w = bits.cpu().numpy(), best.cpu().numpy()
    assert (b[:GUARD] == gb).all() and (b[-GUARD:] == gb).all(), "guard words around bits"
    assert (w[:GUARD] == gw).all() and (w[-GUARD:] == gw).all(), "guard words around best"
    if not want_best:
        assert (w == gw).all(), "best is NULL: nothing but bits may be written"
    return b[GUARD:-GUARD].view(np.uint64).reshape(nf, nc), (w[GUARD:-GUARD].astype(np.uint32) if want_best else None)
