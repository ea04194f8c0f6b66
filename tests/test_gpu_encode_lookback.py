"""encode_kernel's look-back (enc_kernel.h calling the shared protocol of
enc_common.h: lb_prefetch, lb_scalar, lb_resolve, lb_tail_wait; DESIGN.md 3.1
step 4) at the small shapes where it changes path, against the oracle's
per-frame compress, bit-exact with the identifier bytes 8-13 masked.

encode_kernel serves what the fast kernels refuse, so every case here is
refused by them for one reason (k = 8 > 7, MULTI, a g that is no power of two,
partial or unaligned frames, 32-bit samples, a MODEL batch the walks do not
take), and every test asserts through the device layer's launch counters
(airs_dev_launch_stats) that its call was encode_kernel launches and nothing
else: a shape that quietly goes to another kernel fails here.

Segments are 16384 samples for 16-bit frames and 8192 for 32-bit samples and
MODEL launches; sif is the segment's index in its frame.  Where the look-back
overlaps the packing (every case but partial MODEL frames), segments with
sif >= 16 read their first window through scalar loads (16 granules; the
lanes above read as unpublished), the others through vector loads issued a
chunk earlier; further windows are vector loads of 64 granules.

  frames x segments
   3 x 16   sif < 16 everywhere: the prefetched vector window only
   3 x 17   the first scalar round, its window starting at the frame's first granule
   3 x 18   the second
   2 x 66   a scalar round followed by vector windows, the last one clamped at
            the frame's first granule
   2 x 130  three vector windows

`mixed` frames (rice_helpers.pool_frames) put constant, laplace and uniform
segments side by side: a slow predecessor in front of fast successors gives
the re-poll branch of lb_resolve a chance to run.  No test can force it: which
granule is published when a window is read is up to the hardware's timing."""
import zlib

import numpy as np
import pytest

import streams
from conftest import load_pkg
from rice_helpers import ENCODE, ENCODE_STREAM, SEG, Launches, compare, gpu, mask, oracle, pool_frames

pytestmark = pytest.mark.gpu
pkg = load_pkg()
api = pkg.cmpapi
P = api.CmpParams
SEG32 = 8192  # samples per segment: 32-bit samples, MODEL launches
G8 = 256      # GOLOMB_ZERO g = 2^8: past the Rice kernel's k <= 7


@pytest.fixture(scope="module")
def eng(prod):
    if not prod.gpu_available():
        pytest.fail("GPU test run without a usable HIP device")
    e = prod.engine()
    yield e
    e.close()


def _kind(pre, spf):
    return "u16" if (pre + spf) % 2 == 0 else "i16"


def _rng(*key):
    return np.random.default_rng(zlib.crc32("/".join(str(k) for k in key).encode()))


# ---- a. the window shapes, GOLOMB_ZERO g = 256 --------------------------------

SHAPES = ((3, 16), (3, 17), (3, 18), (2, 66), (2, 130))


@pytest.mark.parametrize("pre", (0, 1))
@pytest.mark.parametrize("nf,spf", SHAPES)
def test_encode_lookback_shapes(prod, eng, orc, nf, spf, pre):
    kind = _kind(pre, spf)
    checksum = (spf + pre) % 3 == 0
    for data in ("mixed", ("laplace", "outliers")[(spf + pre) % 2]):
        frames = pool_frames(_rng("shapes", nf, spf, pre, data), kind, nf, spf, 8, data)
        want = oracle(orc, kind, pre, G8, frames, checksum)
        with Launches(prod) as l:
            got = gpu(prod, eng, kind, pre, G8, frames, checksum)
        l.only(ENCODE, 1)
        compare(orc, kind, pre, G8, frames, got, want, f"{nf}x{spf} pre={pre} {data} checksum={checksum}")


# ---- b. the other coders, partial and unaligned frames, 32-bit samples --------

def _oracle(orc, kind, prm, frames):
    """The oracle's compress of every frame, each on a fresh context."""
    want = []
    for x in frames:
        ctx = api.CmpContext()
        assert not api.is_error(orc.initialise(ctx, prm))
        cap = orc.compress_bound(2 * x.size)
        dst = api.aligned_empty(cap)
        r = orc.compress(kind, ctx, dst, cap, x)
        assert not api.is_error(r), api.error_name(r)
        want.append(bytes(dst[:r]))
    return want


def _gpu(prod, eng, kind, prm, frames, flags=0, src_offset=0):
    """One cmp_gpu_compress call, one context: the frames' bytes."""
    import torch
    n, nf = frames[0].size, len(frames)
    sb = 4 if kind == "i16_in_i32" else 2
    stride = (n * sb + 15) // 16 * 16
    host = np.zeros(src_offset + nf * stride + 16, dtype=np.uint8)
    for f, x in enumerate(frames):
        host[src_offset + f * stride:src_offset + f * stride + n * sb] = np.ascontiguousarray(x).view(np.uint8)
    src = torch.from_numpy(host).cuda()
    cap = prod.compress_bound(2 * n)
    dstride = (cap + 7) // 8 * 8
    dst = torch.full((nf * dstride,), 0xAB, dtype=torch.uint8, device="cuda")
    sizes = torch.zeros(nf, dtype=torch.int32, device="cuda")
    ctxs = (api.CmpContext * 1)()
    assert not api.is_error(prod.initialise(ctxs[0], prm))
    torch.cuda.synchronize()
    r = eng.compress(ctxs, nf, kind, src.data_ptr() + src_offset, stride, n * sb, dst.data_ptr(), dstride, cap,
                     sizes.data_ptr(), flags)
    assert r == 0, api.error_name(r)
    assert eng.synchronize() == 0
    sz = sizes.cpu().numpy().astype(np.uint32)
    out = dst.cpu().numpy()
    got = []
    for f in range(nf):
        assert not api.is_error(int(sz[f])), (f, api.error_name(int(sz[f])))
        got.append(bytes(out[f * dstride:f * dstride + int(sz[f])]))
    return got


def _same(got, want, note):
    bad = [f for f in range(len(want)) if mask(got[f]) != mask(want[f])]
    assert not bad, (note, bad, [(len(got[f]), len(want[f])) for f in bad])


def _wide(rng, frames):
    """16-bit patterns as i16 in i32: junk in the high half, which the encoder ignores."""
    return [(x.astype(np.int64) | (rng.integers(-30000, 30000, x.size) << 16)).astype(np.int32) for x in frames]


N18 = 18 * SEG
VARIANTS = {
    # name: (sample kind, samples per frame, source offset, encoder, g, outlier)
    "multi_g8": ("u16", N18, 0, api.ENCODER_GOLOMB_MULTI, 8, 107),  # the second coder family
    "zero_g24": ("i16", N18, 0, api.ENCODER_GOLOMB_ZERO, 24, 0),    # the non-Rice golomb path
    "n_minus_2": ("u16", N18 - 2, 0, api.ENCODER_GOLOMB_ZERO, G8, 0),  # no whole segments: the non-FULL kernel
    "src_offset_2": ("i16", N18, 2, api.ENCODER_GOLOMB_ZERO, G8, 0),   # frames not 16-byte aligned: the same
    "wide": ("i16_in_i32", 18 * SEG32, 0, api.ENCODER_GOLOMB_ZERO, 32, 0),  # 32-bit samples: 8192 per segment
}


@pytest.mark.parametrize("pre", (0, 1))
@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_encode_lookback_variants(prod, eng, orc, name, pre):
    """3 frames x 18 segments (the second scalar round) through the kernel's
    other instantiations."""
    kind, n, off, enc, g, outl = VARIANTS[name]
    rng = _rng("variants", name, pre)
    frames = [x[:n] for x in pool_frames(rng, "i16" if kind == "i16" else "u16", 3, -(-n // SEG), 5, "mixed")]
    if kind == "i16_in_i32":
        frames = _wide(rng, frames)
    prm = P(primary_preprocessing=pre, primary_encoder_type=enc, primary_encoder_param=g,
            primary_encoder_outlier=outl, checksum_enabled=pre)
    want = _oracle(orc, kind, prm, frames)
    with Launches(prod) as l:
        got = _gpu(prod, eng, kind, prm, frames, src_offset=off)
    l.only(ENCODE, 1)
    _same(got, want, (name, pre))


# ---- c. a payload-only stream -------------------------------------------------

@pytest.mark.parametrize("pre", (0, 1))
@pytest.mark.parametrize("nseg", (18, 66))
def test_encode_lookback_stream(prod, eng, nseg, pre):
    """cmp_gpu_encode_stream with g = 256: encode_kernel in STREAM mode (no
    header, the first payload bit at bit 0), one look-back chain."""
    from test_gpu_stream import gpu_stream
    kind = _kind(pre, nseg)
    x = pool_frames(_rng("stream", nseg, pre), kind, 1, nseg, 8, "mixed")[0]
    want = streams.oracle_stream(x, kind, pre, api.ENCODER_GOLOMB_ZERO, G8, 0)
    with Launches(prod) as l:
        got = gpu_stream(eng, x, kind, pre, api.ENCODER_GOLOMB_ZERO, G8, 0)
    l.only(ENCODE_STREAM, 1)
    assert got == want, (nseg, pre, got[0], want[0])


# ---- d. the fused Rice selection: the tail-only wait --------------------------

@pytest.mark.parametrize("pre", (0, 1))
def test_encode_lookback_fused_selection(prod, eng, orc, orc_ext, pre):
    """CMP_GPU_AUTO_RICE on 8 frames of 8 segments less 2 samples: partial
    segments keep the batch off the Rice kernel, and encode_kernel's fused
    selection knows every offset from the candidate granules, so a segment
    waits for its predecessor's tail granule only (lb_tail_wait)."""
    from test_gpu_autorice import _oracle as auto_oracle
    kind = _kind(pre, 8)
    frames = [x[:8 * SEG - 2] for x in pool_frames(_rng("fused", pre), kind, 8, 8, 3 + pre, "mixed")]
    want = auto_oracle(orc, orc_ext, kind, pre, frames, checksum=pre)
    prm = P(primary_preprocessing=pre, primary_encoder_type=api.ENCODER_GOLOMB_ZERO, primary_encoder_param=7,
            checksum_enabled=pre)  # (the configured g is ignored)
    with Launches(prod) as l:
        got = _gpu(prod, eng, kind, prm, frames, flags=pkg.GPU_AUTO_RICE)
    l.only(ENCODE, 1)  # not RICE_AUTO
    _same(got, want, ("fused", pre))


# ---- e. a MODEL batch the walks refuse ----------------------------------------

@pytest.mark.parametrize("kind", ("u16", "i16_in_i32"))
def test_encode_lookback_model_batch(prod, eng, orc, kind):
    """One context, three frames of 17 segments of 8192 samples (a primary
    pass, then two MODEL passes), the secondary g no power of two: neither
    walk takes the batch, and each acquisition step is one encode_kernel
    launch of whole, aligned frames at the worst-case capacity, whose look-back
    overlaps the packing like a frame's without a model.  Against the call
    loop on the oracle: frames, context state and work buffer."""
    from test_gpu_walk import make_frames, run_gpu, run_host
    n = 17 * SEG32
    prm = P(primary_preprocessing=1, primary_encoder_type=api.ENCODER_GOLOMB_ZERO, primary_encoder_param=16,
            secondary_iterations=4, secondary_preprocessing=3, secondary_encoder_type=api.ENCODER_GOLOMB_MULTI,
            secondary_encoder_param=24, secondary_encoder_outlier=107, model_rate=11, checksum_enabled=1,
            uncompressed_fallback_enabled=0)
    calls = [(3, make_frames(kind, n, 3, _rng("model", kind)))]
    cap = 26 + 6 * n
    want = run_host(orc, [prm], kind, n, 1, calls, cap)
    with Launches(prod) as l:
        got = run_gpu(prod, eng, [prm], kind, n, 1, calls, cap)
    l.only(ENCODE, 3)
    assert got == want
