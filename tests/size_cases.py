"""Frames of exact size, from code-length arithmetic alone (no GPU).

Every encode route ends in a comparison of a frame's size with a limit (the
destination capacity, the raw frame size of the uncompressed fallback, the
24-bit size field, the bit at which a MODEL pass stops updating its model).
The builders here make samples whose frame has exactly a wanted number of
payload bits, so a test can put a frame on the limit, one byte below and one
above.

Only the code LENGTH of a mapped value is restated (reference
lib/compress/encoder.c:63-224, 303-378: GOLOMB_ZERO and GOLOMB_MULTI at any
g); what the bits are is left to the oracle.  Every user asserts with
`oracle_size` that the oracle returns the intended size at full capacity, so a
wrong restatement stops the test instead of weakening it.

    lengths = length_table(enc, g, outlier)      # per mapped value 0 .. 65535
    lens = spread(lengths, n, bits, rng)         # n code lengths, sum == bits
    m = mapped_with(lengths, lens, rng)          # mapped values of these lengths
    x = samples(kind, pre, m, rng, model=...)    # u16 / i16 / i16_in_i32 samples
"""
import numpy as np

NONE, DIFF, IWT, MODEL = range(4)
UNCOMPRESSED, ZERO, MULTI = range(3)
HDR, HDR_EXT, CK = 16, 22, 4


def length_table(enc, g, outlier=0):
    """Code length in bits of every mapped (zigzag) value 0 .. 65535."""
    m = np.arange(65536, dtype=np.int64)
    if enc == UNCOMPRESSED:
        return np.full(65536, 16, dtype=np.int64)
    assert enc in (ZERO, MULTI) and 1 <= g <= 0xFFFF
    k = int(g).bit_length() - 1
    cutoff = (2 << k) - g
    limit = cutoff + (31 - k) * g  # first value whose codeword would exceed 32 bits
    if enc == MULTI:
        limit = max(limit - 8, 0)
        want = outlier
    else:
        want = min(cutoff + 16 * g - 1, 0xFFFFFFFF)
    outl = min(want, limit)
    assert outl > 0

    def golomb(v):
        return np.where(v < cutoff, k + 1, k + 2 + (np.maximum(v, cutoff) - cutoff) // g)

    if enc == ZERO:
        return np.where(m < outl, golomb(m + 1), k + 17)
    d = np.maximum(m - outl, 0)
    lvl = np.where(d < 4, 0, (np.floor(np.log2(np.maximum(d, 1))).astype(np.int64)) // 2)
    return np.where(m < outl, golomb(m), golomb(outl + lvl) + 2 * (lvl + 1))


def escape_pieces(enc, g, outlier, m):
    """(bits of the first piece, bits of the second) of GOLOMB_MULTI's escape
    for mapped value m >= outlier: the escape symbol's codeword, then the raw
    difference (encoder.c:358-371: two writes)."""
    assert enc == MULTI
    t = length_table(enc, g, outlier)
    k = int(g).bit_length() - 1
    cutoff = (2 << k) - g
    outl = min(outlier, max(cutoff + (31 - k) * g - 8, 0))
    assert m >= outl
    d = m - outl
    lvl = 0 if d < 4 else (int(d).bit_length() - 1) // 2
    second = 2 * (lvl + 1)
    return int(t[m]) - second, second


def run_of_lengths(lengths):
    """(lo, hi): the longest run of consecutive integers among the table's
    code lengths (GOLOMB_ZERO at g = 2^k: k+2 .. k+17)."""
    have = sorted(set(int(v) for v in lengths))
    best, lo = (have[0], have[0]), have[0]
    for a, b in zip(have, have[1:] + [None]):
        if b != a + 1:
            if a - lo > best[1] - best[0]:
                best = (lo, a)
            lo = b
    return best


def spread(lengths, n, bits, rng, jitter=0.5):
    """n code lengths from the table's run of consecutive lengths whose sum is
    exactly `bits`; a `jitter` share of the samples is moved in pairs (+d, -d)
    so that the frame is not two lengths only."""
    lo, hi = run_of_lengths(lengths)
    assert n * lo <= bits <= n * hi, (n, lo, hi, bits)
    base, rem = divmod(bits, n)
    lens = np.full(n, base, dtype=np.int64)
    lens[:rem] += 1
    pairs = int(n * jitter) // 2
    if pairs:
        idx = rng.permutation(n)[:2 * pairs]
        a, b = idx[:pairs], idx[pairs:]
        room = np.minimum(hi - lens[a], lens[b] - lo)
        d = (rng.random(pairs) * (room + 1)).astype(np.int64)
        lens[a] += d
        lens[b] -= d
    rng.shuffle(lens)
    assert int(lens.sum()) == bits and lens.min() >= lo and lens.max() <= hi
    return lens


def mapped_with(lengths, lens, rng):
    """A mapped value of code length lens[i] for every i (uniform among the
    values of that length)."""
    order = np.argsort(lengths, kind="stable")
    sorted_len = lengths[order]
    first = np.searchsorted(sorted_len, lens, side="left")
    last = np.searchsorted(sorted_len, lens, side="right")
    assert (last > first).all(), "a code length the coder does not have"
    pick = first + (rng.random(len(lens)) * (last - first)).astype(np.int64)
    return order[pick]


def residuals(m):
    """The 16-bit residual (as 0 .. 65535) whose zigzag value is m."""
    m = np.asarray(m, dtype=np.int64)
    return ((m >> 1) ^ -(m & 1)) & 0xFFFF


def samples(kind, pre, m, rng, model=None):
    """Samples whose residuals under `pre` map to m.  DIFF: the running sum of
    the residuals; MODEL: the model plus the residuals (after a primary pass
    the model is the previous frame; later it is what the context's work
    buffer holds).  i16_in_i32 samples carry junk upper halves."""
    r = residuals(m)
    if pre == DIFF:
        v = np.cumsum(r) & 0xFFFF
    elif pre == MODEL:
        assert model is not None and len(model) == len(r)
        v = (np.asarray(model).view(np.uint16).astype(np.int64) + r) & 0xFFFF
    else:
        assert pre == NONE
        v = r
    return from_low16(kind, v, rng)


def from_low16(kind, v, rng):
    """Samples of `kind` with the 16-bit patterns v; i16_in_i32 samples carry
    junk upper halves."""
    v = (np.asarray(v, dtype=np.int64) & 0xFFFF).astype(np.uint16)
    if kind == "u16":
        return v
    if kind == "i16":
        return v.view(np.int16)
    assert kind == "i16_in_i32"
    junk = rng.integers(0, 0x10000, len(v)).astype(np.uint32) << 16
    return (junk | v).view(np.int32)


def low16(x):
    """The 16-bit patterns of samples of any kind (what a model stores after a
    primary pass)."""
    x = np.ascontiguousarray(x)
    if x.dtype.itemsize == 4:
        return (x.view(np.uint32) & 0xFFFF).astype(np.uint16)
    return x.view(np.uint16).copy()


def header_size(pre, enc):
    return HDR if (pre == NONE and enc == UNCOMPRESSED) else HDR_EXT


def raw_size(n, checksum):
    """The uncompressed fallback's frame (cmp.c:342-393)."""
    return HDR + 2 * n + (CK if checksum else 0)


def payload_bits(size, pre, enc, checksum, pad=0):
    """Payload bits of a frame of `size` bytes whose last payload byte has
    `pad` (0 .. 7) unused bits."""
    assert 0 <= pad < 8
    body = size - header_size(pre, enc) - (CK if checksum else 0)
    assert body > 0
    return 8 * body - pad


def frame_size(bits, pre, enc, checksum):
    return header_size(pre, enc) + (bits + 7) // 8 + (CK if checksum else 0)


def sized_frame(kind, pre, enc, g, outlier, n, size, checksum, rng, pad=0, model=None, jitter=0.5):
    """Samples of a frame of exactly `size` bytes under (pre, enc, g, outlier)."""
    t = length_table(enc, g, outlier)
    lens = spread(t, n, payload_bits(size, pre, enc, checksum, pad), rng, jitter)
    return samples(kind, pre, mapped_with(t, lens, rng), rng, model)


class Family:
    """Frames of one coder and length that differ by a few bits: a base of n
    code lengths around `bits` (spread), from which frame() moves single
    samples by one bit until the sum is the wanted one.  Cheap where a test
    wants many frames a byte apart.  lo, hi: the lengths frame() stays within
    (default: the table's run of consecutive lengths)."""

    def __init__(self, enc, g, outlier, n, bits, rng, jitter=0.5, lo=None, hi=None):
        self.enc, self.g, self.outlier, self.n = enc, g, outlier, n
        self.table = length_table(enc, g, outlier)
        run = run_of_lengths(self.table)
        self.lo, self.hi = (run[0] if lo is None else lo), (run[1] if hi is None else hi)
        self.lens = spread(self.table, n, bits, rng, jitter)
        assert self.lens.min() >= self.lo and self.lens.max() <= self.hi
        self.m = mapped_with(self.table, self.lens, rng)
        self.bits = bits

    def frame(self, kind, pre, bits, rng, model=None):
        delta = bits - self.bits
        lens, m = self.lens, self.m
        if delta:
            step = 1 if delta > 0 else -1
            ok = np.flatnonzero((lens + step >= self.lo) & (lens + step <= self.hi))
            idx = rng.choice(ok, abs(delta), replace=False)
            lens, m = lens.copy(), m.copy()
            lens[idx] += step
            m[idx] = mapped_with(self.table, lens[idx], rng)
            assert int(lens.sum()) == bits
        return samples(kind, pre, m, rng, model)


def replay(orc, api, kind, params, frames, cap=None, primary_g=None):
    """The frames in order on a fresh context of the oracle at capacity cap
    (default: the worst case): [(return value, model after the call as uint16
    or None)]."""
    sb = 4 if kind == "i16_in_i32" else 2
    n = len(frames[0])
    w = orc.cal_work_buf_size(params, n * sb)
    assert not api.is_error(w)
    buf = api.aligned_empty(max(w, 2), fill=0)
    ctx = api.CmpContext()
    r = orc.initialise(ctx, params, buf if w else None, w)
    assert not api.is_error(r), api.error_name(r)
    cap = 26 + 6 * n if cap is None else cap
    dst = api.aligned_empty(cap)
    out = []
    for f in frames:
        if primary_g is not None:
            ctx.params.primary_encoder_param = primary_g(f)
        r = orc.compress(kind, ctx, dst, cap, f)
        out.append((r, buf[:2 * n].view(np.uint16).copy() if w else None))
    return out


def oracle_size(orc, api, kind, params, x, prior=()):
    """The oracle's return for x at full capacity on a fresh context, after
    the frames of `prior` (also at full capacity): the self-check of a case.
    Returns (size, model after the call as uint16 or None)."""
    return replay(orc, api, kind, params, tuple(prior) + (x,))[-1]
