"""The Rice/ZERO frame kernel's fixed per-segment work (enc_rice.hip,
DESIGN.md 3.1.5) at the smallest shapes that reach it, bit-exact against the
oracle, each case asserting its kernel and look-back mode through the launch
counters:

  * the wave totals after B1, formed in scalar code from the four waves' sums
    (chunk totals that differ by wave, totals past 2^16 bits, the chunk-by-chunk
    path of a segment that does not fit the arena);
  * the scalar look-back in windows of 8 granules (frames of 17 and 18
    segments under lbmode 1: sif 16 walks two windows, sif 17 three, the last
    one clamped at the frame's first granule);
  * the segment's last 32 bits, formed in scalar code from lane 63's eight
    pairs, with the vector path kept for a pair of lane 63 over 32 bits.

About the tail cases.  A codeword has at least two bits at every k (k = 0:
v = m + 1 >= 1 gives q >= 1, length 1 + q; k >= 1: length k + 1), so lane 63's
16 samples hold at least 32 bits: a chunk of fewer bits, for which the tail
would reach into lanes 60-62, cannot be made from any input.  The cases here
are the nearest ones that exist: all-zero residuals at k = 0 and k = 1 (lane 63
holds exactly 32 bits, the whole tail word is its own), 33 bits at k = 1 (one
bit of the word comes from the 15th sample back), and two escapes in lane 63's
last and in its first pair (pairs of 2 (k + 17) > 32 bits: the vector path).
Every pattern is laid over the last 64 samples of EVERY segment, the frame's
last one (which publishes no tail) included, in frames of two segments, so
that segment 1 shifts segment 0's tail into its first word."""
import zlib

import numpy as np
import pytest

import streams
from conftest import load_pkg
from rice_helpers import (LB0, LB1, RICE_AUTO, RICE_STREAM, SEG, Launches, as_kind, compare, gpu, mask, oracle,
                          pool, pool_frames)

pytestmark = pytest.mark.gpu
api = load_pkg().cmpapi
CHUNK = SEG // 4   # samples per chunk: lane t of the workgroup owns [16 t, 16 t + 16)
WAVE = CHUNK // 4  # samples of one wave in a chunk


@pytest.fixture(scope="module")
def eng(prod):
    if not prod.gpu_available():
        pytest.fail("GPU test run without a usable HIP device")
    e = prod.engine()
    yield e
    e.close()


def _mode(nf):
    return LB1 if nf % 8 == 0 else LB0


def _run(prod, eng, orc, kind, pre, k, frames, checksum, note):
    want = oracle(orc, kind, pre, 1 << k, frames, checksum)
    with Launches(prod) as l:
        got = gpu(prod, eng, kind, pre, 1 << k, frames, checksum)
    l.only(_mode(len(frames)), 1)
    compare(orc, kind, pre, 1 << k, frames, got, want, note)


# ---- a. frames and modes ----------------------------------------------------

@pytest.mark.parametrize("k", (0, 1, 5, 7))
@pytest.mark.parametrize("nf", (8, 7))
@pytest.mark.parametrize("spf", (1, 2, 17, 18))
def test_fixed_work_shapes(prod, eng, orc, spf, nf, k):
    """NONE and DIFF, with and without checksum (every (pre, checksum) pair
    per shape and k), laplace noise at the scale of g: 17 segments reach the
    scalar look-back under 8 frames, 18 walk past an 8-granule window."""
    for pre in (0, 1):
        for checksum in (0, 1):
            rng = np.random.default_rng(zlib.crc32(f"fw/{spf}/{nf}/{k}/{pre}/{checksum}".encode()))
            kind = "u16" if (k + pre) % 2 == 0 else "i16"
            frames = pool_frames(rng, kind, nf, spf, k, "laplace")
            _run(prod, eng, orc, kind, pre, k, frames, checksum, f"{nf}x{spf} k={k} pre={pre} ck={checksum}")


# ---- b. the segment's last 32 bits -----------------------------------------

def _unmap(m):
    """The 16-bit sample whose ZigZag value is m (NONE)."""
    m = np.asarray(m, dtype=np.int64)
    return np.where(m % 2 == 0, m // 2, -(m + 1) // 2)


def _tail(pattern, pre, k):
    """The last 64 samples of a segment (lanes 60-63 of wave 3, chunk 3)."""
    if pre == 0:
        m = np.zeros(64, dtype=np.int64)
        if pattern == "bits33":
            assert k == 1
            m[49] = 1  # v = 2: q = 1, three bits; the other 15 samples of lane 63 two each
        elif pattern == "esc_last":
            m[62:64] = (65535, 40000)
        elif pattern == "esc_first":
            m[48:50] = (40000, 65535)
        else:
            assert pattern == "zeros"
        return _unmap(m)
    x = np.full(64, 1234, dtype=np.int64)  # DIFF: a constant run, residual 0 from its second sample on
    if pattern == "esc_last":
        x[62] += 20000  # residuals +20000, -20000: samples 62 and 63, one pair
    elif pattern == "esc_first":
        x[48] += 20000
    else:
        assert pattern == "zeros"
    return x


TAILS = [("zeros", 0, 0), ("zeros", 0, 1), ("bits33", 0, 1), ("zeros", 1, 0), ("zeros", 1, 5),
         ("esc_last", 0, 0), ("esc_last", 0, 7), ("esc_first", 0, 1), ("esc_first", 0, 5),
         ("esc_last", 1, 1), ("esc_last", 1, 5), ("esc_first", 1, 0), ("esc_first", 1, 7)]


@pytest.mark.parametrize("nf", (8, 7))
@pytest.mark.parametrize("pattern,pre,k", TAILS)
def test_fixed_work_tail(prod, eng, orc, pattern, pre, k, nf):
    rng = np.random.default_rng(zlib.crc32(f"tail/{pattern}/{pre}/{k}/{nf}".encode()))
    kind = "i16"
    frames = []
    for f in pool_frames(rng, kind, nf, 2, k, "laplace"):
        x = f.astype(np.int64)
        for s in range(2):
            x[(s + 1) * SEG - 64:(s + 1) * SEG] = _tail(pattern, pre, k)
        frames.append(as_kind(x, kind))
    # segment 1 must not start on a word boundary in every frame (its first
    # word then takes no bit of the tail): the noise before the pattern sees to it
    _run(prod, eng, orc, kind, pre, k, frames, nf == 7, f"tail {pattern} pre={pre} k={k} nf={nf}")


# ---- c. the wave totals ----------------------------------------------------

def _wave_frames(nf, spf, what):
    frames = []
    for f in range(nf):
        m = np.zeros(spf * SEG, dtype=np.int64)
        for s in range(spf):
            for c in range(4):
                if what == "one_wave":
                    # chunk c: wave (c + s + f) mod 4 all escapes (17 bits a sample at
                    # k = 0), the other three zeros (2 bits): every wave offset differs
                    w = (c + s + f) % 4
                    o = s * SEG + c * CHUNK + w * WAVE
                    m[o:o + WAVE] = 65535 - (np.arange(WAVE) % 7)
                else:  # every sample an escape: 17 bits x 16384 do not fit the arena
                    m[s * SEG:(s + 1) * SEG] = 65535 - (np.arange(SEG) % 5)
        frames.append(as_kind(_unmap(m), "i16"))
    return frames


@pytest.mark.parametrize("nf,spf", ((8, 2), (7, 2), (8, 17)))
@pytest.mark.parametrize("what", ("one_wave", "all_escape"))
def test_fixed_work_wave_totals_constant_runs(prod, eng, orc, what, nf, spf):
    """NONE, k = 0, constant runs: `one_wave` fits the arena (94 208 bits a
    segment), `all_escape` does not (278 528 bits) and is stored chunk by
    chunk, its look-back at the second call site."""
    _run(prod, eng, orc, "i16", 0, 0, _wave_frames(nf, spf, what), spf == 17, f"{what} {nf}x{spf}")


@pytest.mark.parametrize("nf", (8, 7))
@pytest.mark.parametrize("pre", (0, 1))
def test_fixed_work_wave_totals_past_16_bits(prod, eng, orc, pre, nf):
    """Uniform noise at k = 7: about 24 bits a sample, so a chunk's total over
    the four waves (~98 000 bits) passes 2^16 while each wave's own sum stays
    below it (the halves of the packed wave sums are added in 32 bits)."""
    rng = np.random.default_rng(900 + 2 * nf + pre)
    frames = pool_frames(rng, "u16", nf, 2, 7, "uniform")
    _run(prod, eng, orc, "u16", pre, 7, frames, pre, f"uniform k=7 pre={pre} nf={nf}")


# ---- d. the payload-only stream --------------------------------------------

@pytest.mark.parametrize("pre,k", ((0, 0), (1, 1), (1, 5), (0, 7)))
def test_fixed_work_stream(prod, eng, pre, k):
    """One stream of 18 segments (rice_kernel<PRE, true>, the vector
    look-back), the tail patterns laid over some of its segments."""
    import torch
    rng = np.random.default_rng(70 + k)
    off = int(rng.integers(0, pool(k, "laplace").size - 18 * SEG))
    x = pool(k, "laplace")[off:off + 18 * SEG].view(np.int16).astype(np.int64)
    for s, pattern in ((2, "zeros"), (5, "esc_last"), (9, "esc_first"), (16, "esc_last"), (17, "zeros")):
        x[(s + 1) * SEG - 64:(s + 1) * SEG] = _tail(pattern, pre, k)
    x = as_kind(x, "i16")
    want = streams.oracle_stream(x, "i16", pre, 1, 1 << k, 0)
    cap = 6 * x.size + 64
    src = torch.from_numpy(x.view(np.uint8).copy()).cuda()
    dst = torch.full(((cap + 64 + 7) // 8 * 8,), 0xAB, dtype=torch.uint8, device="cuda")
    size = torch.zeros(1, dtype=torch.int32, device="cuda")
    with Launches(prod) as l:
        assert eng.encode_stream("i16", src.data_ptr(), x.size, pre, 1, 1 << k, 0, dst.data_ptr(), cap,
                                 size.data_ptr()) == 0
        assert eng.synchronize() == 0
    l.only(RICE_STREAM, 1)
    s = int(size.cpu().numpy().astype(np.uint32)[0])
    assert not api.is_error(s), api.error_name(s)
    assert (s, bytes(dst[:s].cpu().numpy())) == want


# ---- e. AUTO ----------------------------------------------------------------

@pytest.mark.parametrize("pre", (0, 1))
def test_fixed_work_auto(prod, eng, orc, orc_ext, pre):
    """cfg3's shape, 8 frames of 4 segments with the frame's k chosen in the
    kernel (rice_kernel<PRE, false, true> shares the wave totals and the
    tail): noise of another scale per frame, the tail patterns on segment 1."""
    import torch
    n, nf, kind = 4 * SEG, 8, "i16"
    frames = []
    for f in range(nf):
        x = pool(f % 8, "laplace")[f * 4099:f * 4099 + n].view(np.int16).astype(np.int64)
        x[2 * SEG - 64:2 * SEG] = _tail(("zeros", "esc_last", "esc_first")[f % 3], pre, 0)
        frames.append(as_kind(x, kind))
    want = []
    for x in frames:
        k = orc_ext.orc_select_rice_k(np.ascontiguousarray(x).ctypes.data, n, 0, pre, None)
        want += oracle(orc, kind, pre, 1 << k, [x], 0)
    host = np.concatenate([x.view(np.uint8) for x in frames])
    src = torch.from_numpy(host).cuda()
    cap = prod.compress_bound(2 * n)
    dstride = (cap + 7) // 8 * 8
    dst = torch.full((nf * dstride,), 0xAB, dtype=torch.uint8, device="cuda")
    sizes = torch.zeros(nf, dtype=torch.int32, device="cuda")
    ctxs = (api.CmpContext * 1)()
    assert not api.is_error(prod.initialise(ctxs[0], api.CmpParams(
        primary_preprocessing=pre, primary_encoder_type=api.ENCODER_GOLOMB_ZERO, primary_encoder_param=7)))
    torch.cuda.synchronize()
    with Launches(prod) as l:
        assert eng.compress(ctxs, nf, kind, src.data_ptr(), 2 * n, 2 * n, dst.data_ptr(), dstride, cap,
                            sizes.data_ptr(), 1) == 0
        assert eng.synchronize() == 0
    l.only(RICE_AUTO, 1)
    sz = sizes.cpu().numpy().astype(np.uint32)
    out = dst.cpu().numpy()
    for f in range(nf):
        assert not api.is_error(int(sz[f])), (f, api.error_name(int(sz[f])))
        got = bytes(out[f * dstride:f * dstride + int(sz[f])])
        assert mask(got) == mask(want[f]), (f, len(got), len(want[f]))
