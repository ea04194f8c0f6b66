"""The Rice kernel's front block (enc_rice.hip): the block
index is turned into (segment in frame, launch frame) by multiplications with
the host's reciprocals, from one 64-byte read of the kernel arguments.
Bit-exact against the oracle at the smallest shapes where that index
arithmetic can go wrong:

  * frame counts 1, 3, 5, 7, 8, 9 and 24 (non-powers of two, both sides of a
    multiple of 8: both look-back modes, asserted through the launch counters
    as in test_gpu_rice_lookback.py) with 1, 2, 17 and 18 segments per frame,
    DIFF and NONE, k = 0 and 5;
  * AUTO with 7, 9 and 17 frames of 4 segments: the grid is padded to groups of
    8 frames, so padding blocks take the `lf >= nfr` return;
  * one payload-only stream of 18 segments (one frame: the divisor 1);
  * two launches back to back on one engine with 5 and then 8 frames: a
    reciprocal kept from the launch before would show.

Not covered: a device-planned batch whose launch list has a hole
(AIRS_NO_FRAME).  The scenarios of tests/batch_scenarios.py have frames of at
most 9000 samples, and the Rice kernel takes whole 16 Ki-sample segments only,
so none of them reaches it.

The frames of a (segments, k, preprocessing) combination are the first nf of
one list of 24, so the oracle encodes each list once."""
import zlib

import numpy as np
import pytest

import streams
from conftest import load_pkg
from rice_helpers import LB0, LB1, RICE_AUTO, RICE_STREAM, SEG, Launches, compare, gpu, oracle, pool, pool_frames

pytestmark = pytest.mark.gpu
api = load_pkg().cmpapi

NFS = (1, 3, 5, 7, 8, 9, 24)
SPFS = (1, 2, 17, 18)


@pytest.fixture(scope="module")
def eng(prod):
    if not prod.gpu_available():
        pytest.fail("GPU test run without a usable HIP device")
    e = prod.engine()
    yield e
    e.close()


def _kind(k, pre):
    return "u16" if (k + pre) % 2 == 0 else "i16"


_CACHE = {}


def _frames_and_want(orc, spf, k, pre):
    """max(NFS) frames of spf segments and the oracle's bytes of each
    (checksums on), made once per combination and left unchanged"""
    if (spf, k, pre) not in _CACHE:
        rng = np.random.default_rng(zlib.crc32(f"front/{spf}/{k}/{pre}".encode()))
        kind = _kind(k, pre)
        frames = pool_frames(rng, kind, max(NFS), spf, k, "mixed" if spf >= 3 else "laplace")
        _CACHE[(spf, k, pre)] = (kind, frames, oracle(orc, kind, pre, 1 << k, frames, 1))
    return _CACHE[(spf, k, pre)]


@pytest.mark.parametrize("k", (0, 5))
@pytest.mark.parametrize("pre", (0, 1))
@pytest.mark.parametrize("spf", SPFS)
@pytest.mark.parametrize("nf", NFS)
def test_front_frames_by_segments(prod, eng, orc, nf, spf, pre, k):
    kind, frames, want = _frames_and_want(orc, spf, k, pre)
    with Launches(prod) as l:
        got = gpu(prod, eng, kind, pre, 1 << k, frames[:nf], 1)
    l.only(LB1 if nf % 8 == 0 else LB0, 1)
    compare(orc, kind, pre, 1 << k, frames[:nf], got, want[:nf], f"{nf}x{spf} k={k} pre={pre}")


@pytest.mark.parametrize("pre", (0, 1))
@pytest.mark.parametrize("nf", (7, 9, 17))
def test_front_auto_padded_grid(prod, eng, orc, orc_ext, nf, pre):
    """AUTO: frames of 4 segments, the k chosen in the kernel; 7, 9 and 17
    frames leave 1, 7 and 7 padding frames in the grid's last group of 8."""
    import test_gpu_autorice as ar
    rng = np.random.default_rng(zlib.crc32(f"front/auto/{nf}/{pre}".encode()))
    frames = ar._frames(rng, "u16", 4 * SEG, nf, extreme=True)
    want = ar._oracle(orc, orc_ext, "u16", pre, frames)
    with Launches(prod) as l:
        got = ar._gpu(prod, eng, "u16", pre, frames)
    l.only(RICE_AUTO, 1)
    bad = [f for f in range(nf) if ar._mask(got[f]) != ar._mask(want[f])]
    assert not bad, (nf, pre, bad, [(len(got[f]), len(want[f])) for f in bad[:4]])


def test_front_stream_18_segments(prod, eng):
    from test_gpu_stream import gpu_stream
    k, pre = 5, 1
    x = pool(k, "laplace")[12345:12345 + 18 * SEG]
    want = streams.oracle_stream(x, "u16", pre, 1, 1 << k, 0)  # (size, bytes)
    with Launches(prod) as l:
        got = gpu_stream(eng, x, "u16", pre, 1, 1 << k, 0)
    l.only(RICE_STREAM, 1)
    assert not api.is_error(got[0]), api.error_name(got[0])
    assert got == want, (got[0], want[0])


@pytest.mark.parametrize("pre", (0, 1))
def test_front_back_to_back_frame_counts(prod, orc, pre):
    """5 frames, then 8, then 5 again on one engine of its own: every launch
    carries its own divisors."""
    if not prod.gpu_available():
        pytest.fail("GPU test run without a usable HIP device")
    k, spf = 5, 18
    kind, frames, want = _frames_and_want(orc, spf, k, pre)
    e = prod.engine()
    try:
        for nf, first in ((5, 0), (8, 5), (5, 13)):
            fr, wa = frames[first:first + nf], want[first:first + nf]
            with Launches(prod) as l:
                got = gpu(prod, e, kind, pre, 1 << k, fr, 1)
            l.only(LB1 if nf % 8 == 0 else LB0, 1)
            compare(orc, kind, pre, 1 << k, fr, got, wa, f"back to back {nf}x{spf} pre={pre}")
    finally:
        e.close()
