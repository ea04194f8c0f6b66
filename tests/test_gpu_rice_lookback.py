"""The Rice/ZERO frame kernel's look-back (enc_rice.hip)
at the small shapes where it changes path, against the oracle's per-frame
compress, bit-exact with the identifier bytes 8-13 masked.

A launch whose frame count is a multiple of 8 sets lbmode bit 0; its segments
with sif >= 16 (segment index in the frame) then take rice_lookback_s, the
walk over windows of 16 granules on scalar loads, newest first, clamped at the
frame's first granule, the lanes of a clamped window above the walk's
position masked.  Every other segment, and every segment of a launch with
lbmode 0, takes the vector look-back.  Every test asserts through the device
layer's launch counters (airs_dev_launch_stats) which kernel and which
look-back mode its call took, so a shape that quietly falls back to
encode_kernel, or a changed eligibility rule, fails here.

Frames x segments (of 16384 samples):
   8 x 16  lbmode 1, no segment reaches sif 16: the vector look-back alone
   8 x 17  the first scalar segment: its window's base is the frame's first granule
   8 x 18  sif 17: a second window would be clamped there, lanes above j masked
  16 x 33  three windows
  24 x 20  a frame count that is a multiple of 8 and no power of two
   9 x 18, 7 x 18  lbmode 0 with sif >= 16

`mixed` frames (rice_helpers.pool_frames) put constant, laplace and uniform
segments side by side: a slow predecessor in front of fast successors gives
the re-poll and partial-sum branches of the scalar walk a chance to run (no
test can force them: which granule is published when a window is read is up
to the hardware's timing), and the uniform segments, too large for the arena,
reach the look-back call of the chunk-by-chunk path at sif >= 16 under both
look-back modes.

Not covered here: the vector look-back's take-over after AIRS_RICE_SPOLL
scalar polls (out of reach of a product build), AUTO (test_gpu_autorice.py),
the MODEL walks."""
import zlib

import numpy as np
import pytest

from conftest import load_pkg
from rice_helpers import (ENCODE, HDR, LB0, LB1, SEG, Launches, as_kind, compare, gpu, gpu_raw, mask, oracle,
                          oracle_at, pool_frames)

pytestmark = pytest.mark.gpu
api = load_pkg().cmpapi


@pytest.fixture(scope="module")
def eng(prod):
    if not prod.gpu_available():
        pytest.fail("GPU test run without a usable HIP device")
    e = prod.engine()
    yield e
    e.close()


def _kind(k, pre):
    return "u16" if (k + pre) % 2 == 0 else "i16"


def _mode(nf):
    return LB1 if nf % 8 == 0 else LB0


def _check(prod, eng, orc, nf, spf, k, pre, data, checksum, seed, e=None):
    """One batch of nf frames of spf segments: one launch of the Rice kernel in
    the look-back mode of nf, frames bit-exact."""
    rng = np.random.default_rng(zlib.crc32(f"{nf}x{spf}/{k}/{pre}/{data}/{seed}".encode()))
    kind = _kind(k, pre)
    frames = pool_frames(rng, kind, nf, spf, k, data)
    want = oracle(orc, kind, pre, 1 << k, frames, checksum)
    with Launches(prod) as l:
        got = gpu(prod, e or eng, kind, pre, 1 << k, frames, checksum)
    l.only(_mode(nf), 1)
    compare(orc, kind, pre, 1 << k, frames, got, want, f"{nf}x{spf} k={k} pre={pre} {data} checksum={checksum}")


# ---- a. shapes around the scalar look-back's edges --------------------------

# every (k, pre): mixed data and, in turn, laplace or outliers
EVERY = [(nf, spf, k, pre) for nf, spf in ((8, 18), (16, 33)) for k in range(8) for pre in (0, 1)]
# every k, the preprocessing alternating with k (from another start per shape)
ROTATE = [(nf, spf, k, (k + i) % 2) for i, (nf, spf) in enumerate(((8, 16), (8, 17), (24, 20), (9, 18), (7, 18)))
          for k in range(8)]


@pytest.mark.parametrize("nf,spf,k,pre", EVERY + ROTATE)
def test_lookback_shapes(prod, eng, orc, nf, spf, k, pre):
    checksum = (k + pre + spf) % 3 == 0
    for data in ("mixed", ("laplace", "outliers")[(k + pre + nf // 8) % 2]):
        _check(prod, eng, orc, nf, spf, k, pre, data, checksum, 0)


def test_lookback_shape_table_covers_every_k_and_pre():
    """(the parametrisation above: every shape meets every k and both
    preprocessings; checksums are on for about a third of the cases)"""
    cases = EVERY + ROTATE
    for shape in {(nf, spf) for nf, spf, _, _ in cases}:
        mine = [(k, pre) for nf, spf, k, pre in cases if (nf, spf) == shape]
        assert {k for k, _ in mine} == set(range(8)) and {p for _, p in mine} == {0, 1}, shape
    on = sum((k + pre + spf) % 3 == 0 for _, spf, k, pre in cases)
    assert 0.25 <= on / len(cases) <= 0.42, on


# ---- b. every segment too large for the arena -------------------------------

@pytest.mark.parametrize("nf", (8, 9))
@pytest.mark.parametrize("k,pre", ((0, 1), (3, 0), (5, 1), (7, 0)))
def test_lookback_all_segments_chunked(prod, eng, orc, nf, k, pre):
    """Uniform noise: every segment is stored chunk by chunk after its
    look-back (the second call site), under the scalar (8 frames) and the
    vector (9 frames) look-back."""
    _check(prod, eng, orc, nf, 18, k, pre, "uniform", (k + nf) % 3 == 0, 0)


# ---- c. epoch reuse ---------------------------------------------------------

@pytest.mark.parametrize("k,pre", ((2, 1), (6, 0)))
def test_lookback_epoch_reuse(prod, orc, k, pre):
    """One engine, launch after launch on the same granule arrays: the
    granules of the launch before hold plausible aggregates of the same
    indices under the epoch before, and a scalar walk that took one for its
    own launch's would return a wrong offset.  16 x 33 first (the granule
    arrays are allocated for it, nothing after it reallocates them), 8 x 18
    three times back to back with different data, then a larger (16 x 33) and
    a smaller (8 x 16) launch between further 8 x 18 ones, which shift the
    granule indices against the frame boundaries."""
    if not prod.gpu_available():
        pytest.fail("GPU test run without a usable HIP device")
    e = prod.engine()
    try:
        for i, (nf, spf) in enumerate(((16, 33), (8, 18), (8, 18), (8, 18), (16, 33), (8, 18), (8, 16), (8, 18))):
            _check(prod, None, orc, nf, spf, k, pre, "mixed", i % 3 == 0, i, e=e)
    finally:
        e.close()


# ---- d. capacity clipping in a batch ----------------------------------------

def _clip_frames(k, pre):
    """8 frames of 17 segments, constant (a few KiB coded, DIFF; NONE: values
    below g) and uniform (over 500 KiB coded) in turn."""
    rng = np.random.default_rng(77 + k)
    kind = _kind(k, pre)
    uni = pool_frames(rng, kind, 4, 17, k, "uniform")
    frames = []
    for f in range(8):
        if f % 2:
            frames.append(uni[f // 2])
        else:
            v = int(rng.integers(0, 65536 if pre else 1 << k))
            frames.append(as_kind(np.full(17 * SEG, v), kind))
    return kind, frames


def _clip_run(prod, eng, orc, kind, pre, k, frames, checksum, cap):
    """The batch at capacity cap, one context per frame, against the oracle's
    return at that capacity: status, the bytes of fitting frames, and nothing
    written in [cap, dst_stride).  Returns the number of fitting frames."""
    dstride = (cap + 64 + 7) // 8 * 8
    want = [oracle_at(orc, kind, pre, 1 << k, x, checksum, cap) for x in frames]
    with Launches(prod) as l:
        sz, out = gpu_raw(prod, eng, kind, pre, 1 << k, frames, checksum, cap=cap, dst_stride=dstride,
                          ctx_per_frame=True)
    l.only(LB1, 1)
    note = f"cap={cap} checksum={checksum} k={k} pre={pre}"
    fit = 0
    for f, (r, b) in enumerate(want):
        assert int(sz[f]) == r & 0xFFFFFFFF, (note, f, api.error_name(int(sz[f])), api.error_name(r))
        assert (out[f, cap:] == 0xAB).all(), (note, f, "written past the capacity",
                                              cap + int(np.argmax(out[f, cap:] != 0xAB)))
        if b is not None:
            fit += 1
            compare(orc, kind, pre, 1 << k, [frames[f]], [out[f, :r].tobytes()], [b], f"{note} frame {f}")
    return fit


@pytest.mark.parametrize("k,pre", ((3, 1), (5, 0)))
def test_lookback_capacity_clipping_batch(prod, eng, orc, k, pre):
    """Clipping in a batch of 8 frames x 17 segments whose every other frame
    does not fit.  A capacity below the bound sends the batch through the
    exact-mode path (cmp_batch.c, cmp_gpu_compress); with one context per frame
    and equal parameters that is batch_device_exact, which launches the 8
    frames of an acquisition step together, through a frame list: ONE Rice
    launch with lbmode 1, asserted.  (One context with 8 frames would be 8
    launches of one frame.)  So the segments at sif 16 resolve their offset
    by the scalar walk while the stores of their frame, and of the
    neighbouring frames, are being dropped at the capacity.
    Capacities: one between the two frame sizes; with checksums a constant
    frame's exact size and 1 and 3 bytes less (the checksum's bytes on the
    boundary); 22 (the header), 23 and 24.  Nothing is asserted about the
    bytes below the capacity of a frame that does not fit."""
    kind, frames = _clip_frames(k, pre)
    g = 1 << k
    sizes = [oracle_at(orc, kind, pre, g, x, 0)[0] for x in frames]
    small, large = max(sizes[0::2]), min(sizes[1::2])
    assert small + 4096 + 4 < large
    # between the sizes: the constant frames fit, the uniform ones do not
    assert _clip_run(prod, eng, orc, kind, pre, k, frames, 0, small + 4093) == 4
    assert _clip_run(prod, eng, orc, kind, pre, k, frames, 1, small + 4093) == 4
    # the checksum on the boundary: frame 0's exact size with its checksum, then 1 and 3 bytes less
    s0 = oracle_at(orc, kind, pre, g, frames[0], 1)[0]
    assert s0 == sizes[0] + 4
    assert _clip_run(prod, eng, orc, kind, pre, k, frames, 1, s0) >= 1
    for cap in (s0 - 1, s0 - 3):
        fit = _clip_run(prod, eng, orc, kind, pre, k, frames, 1, cap)
        assert fit < 4  # (frame 0 no longer fits)
    # the header-only edge
    for cap in (HDR, HDR + 1, HDR + 2):
        for checksum in (0, 1):
            assert _clip_run(prod, eng, orc, kind, pre, k, frames, checksum, cap) == 0


# ---- e. dispatch boundaries -------------------------------------------------

N17 = 17 * SEG
DISPATCH = {
    # name: (frames, k, samples per frame, source offset, source stride, the launch expected)
    "k8": (8, 8, N17, 0, 2 * N17, ENCODE),                  # k past the Rice kernel's range
    "n_minus_2": (8, 5, N17 - 2, 0, 2 * N17, ENCODE),       # no whole segments
    "src_offset_2": (8, 5, N17, 2, 2 * N17, ENCODE),        # frames not 16-byte aligned: not FULL
    "src_stride_8": (8, 5, N17, 0, 2 * N17 + 8, ENCODE),    # stride no multiple of 16: not FULL
    "frames_9": (9, 5, N17, 0, 2 * N17, LB0),
    "frames_8": (8, 5, N17, 0, 2 * N17, LB1),
}


@pytest.mark.parametrize("name", sorted(DISPATCH))
@pytest.mark.parametrize("pre", (0, 1))
def test_lookback_dispatch_boundaries(prod, eng, orc, name, pre):
    """The eligibility rules of the Rice kernel around the 8 x 17 shape: which
    kernel family a launch takes, and the same bits either way."""
    nf, k, n, off, stride, expect = DISPATCH[name]
    rng = np.random.default_rng(zlib.crc32(f"dispatch/{name}/{pre}".encode()))
    kind = _kind(k, pre)
    frames = [x[:n] for x in pool_frames(rng, kind, nf, 17, min(k, 7), "mixed")]
    want = oracle(orc, kind, pre, 1 << k, frames, 1)
    with Launches(prod) as l:
        got = gpu(prod, eng, kind, pre, 1 << k, frames, 1, src_offset=off, src_stride=stride)
    l.only(expect, 1)
    bad = [f for f in range(nf) if mask(got[f]) != mask(want[f])]
    assert not bad, (name, bad, [(len(got[f]), len(want[f])) for f in bad])
