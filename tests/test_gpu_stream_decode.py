"""cmp_gpu_decode_stream: payload-only streams (cmp_gpu_encode_stream, no
header) decoded on the GPU.  Streams come from the CPU oracle
(streams.oracle_stream) unless a test says otherwise; they are uploaded to an
8-byte aligned buffer whose bytes past src_size are 0xAB, and decoded into a
buffer with 64 guard samples of 0xA5A5 after num_samples, which every call,
successful or not, must leave intact.  The expected output is the low 16 bits
of the source samples."""
import hashlib

import numpy as np
import pytest

import streams
from conftest import load_pkg

pytestmark = pytest.mark.gpu
api = load_pkg().cmpapi

GUARD = 64
WG_SPAN = 16384  # bytes of stream one parse workgroup owns (256 subsequences of 512 bits)
TILE = 4096  # samples per DIFF-scan tile


@pytest.fixture(scope="module")
def eng(prod):
    if not prod.gpu_available():
        pytest.fail("GPU test run without a usable HIP device")
    e = prod.engine()
    yield e
    e.close()


def low16(x):
    return (np.asarray(x).astype(np.int64) & 0xFFFF).astype(np.uint16)


def upload(data, tail=0xAB):
    """stream bytes -> device buffer (torch allocations are at least 256-byte aligned), padded with `tail`"""
    import torch
    host = np.full((len(data) + 7) // 8 * 8 + 64, tail, dtype=np.uint8)
    host[:len(data)] = np.frombuffer(data, dtype=np.uint8)
    buf = torch.from_numpy(host).cuda()
    assert buf.data_ptr() % 8 == 0
    return buf


def decode_ptr(eng, src_ptr, src_size, n, pre, enc, g, outl, dst_off=0):
    """One call on a device stream.  Returns (call result, *status, the n samples);
    asserts the guard after them (and the samples before an offset dst)."""
    import torch
    dst = torch.full((dst_off // 2 + n + GUARD,), 0xA5A5 - 0x10000, dtype=torch.int16, device="cuda")
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    r = eng.decode_stream(src_ptr, src_size, n, pre, enc, g, outl, dst.data_ptr() + dst_off, st.data_ptr())
    assert eng.synchronize() == 0
    out = dst.cpu().numpy().view(np.uint16)
    assert (out[dst_off // 2 + n:] == 0xA5A5).all(), "guard after num_samples overwritten"
    assert (out[:dst_off // 2] == 0xA5A5).all(), "samples before dst overwritten"
    return r, int(st.cpu().numpy().astype(np.uint32)[0]), out[dst_off // 2:dst_off // 2 + n]


def decode(eng, data, n, pre, enc, g, outl, src_size=None, tail=0xAB, dst_off=0):
    buf = upload(data, tail)
    return decode_ptr(eng, buf.data_ptr(), len(data) if src_size is None else src_size, n, pre, enc, g, outl, dst_off)


def assert_round_trip(eng, x, kind, pre, enc, g, outl, what, **kw):
    size, data = streams.oracle_stream(x, kind, pre, enc, g, outl)
    assert not api.is_error(size), what
    r, st, out = decode(eng, data, x.size, pre, enc, g, outl, **kw)
    assert r == 0, (what, api.error_name(r))
    assert st == x.size, (what, api.error_name(st) if api.is_error(st) else st)
    assert np.array_equal(out, low16(x)), what
    return size, data


def laplace_u16(seed, n, scale=20.0):
    rng = np.random.default_rng(seed)
    v = np.round(rng.laplace(0, scale, n)).astype(np.int64)
    return (v & 0xFFFF).astype(np.uint16)


# ---------------------------------------------------------------- 1. golden
SMALL_GOLD = sorted(k for k, c in streams.GOLD.items() if c["frames"] * c["samples_per_frame"] < (1 << 26))


@pytest.mark.parametrize("name", SMALL_GOLD)
def test_golden_round_trip(eng, name):
    """GPU-encode the case (the bytes are the reference's: size and SHA-256 of
    the golden file), then decode straight from the encoder's device buffer."""
    import torch
    c = streams.GOLD[name]
    x = streams.synth(c)
    n = x.size
    args = (c["preprocessing"], c["encoder_type"], c["encoder_param"], c["encoder_outlier"])
    cap = 6 * n + 64
    src = torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).copy()).cuda()
    enc = torch.full(((cap + 64 + 7) // 8 * 8,), 0xAB, dtype=torch.uint8, device="cuda")
    size = torch.zeros(1, dtype=torch.int32, device="cuda")
    assert eng.encode_stream(c["kind"], src.data_ptr(), n, *args, enc.data_ptr(), cap, size.data_ptr()) == 0
    assert eng.synchronize() == 0
    s = int(size.cpu().numpy().astype(np.uint32)[0])
    assert s == c["size"], (s, c["size"])
    assert hashlib.sha256(bytes(enc[:s].cpu().numpy())).hexdigest() == c["sha256"]
    r, st, out = decode_ptr(eng, enc.data_ptr(), s, n, *args)
    assert r == 0, api.error_name(r)
    assert st == n, api.error_name(st) if api.is_error(st) else st
    assert np.array_equal(out, low16(x))


# ---------------------------------------------------------------- 2. random
def random_cases(count):
    """the generator of test_gpu_stream.py::test_stream_vs_oracle_random"""
    rng = np.random.default_rng(2024)
    seg16, seg32 = 4 * 4096, 2 * 4096
    for t in range(count):
        kind = ["u16", "i16", "i16_in_i32"][t % 3]
        seg = seg32 if kind == "i16_in_i32" else seg16
        n = int(rng.choice([rng.integers(1, 5000), rng.integers(1, 40) * seg,
                            rng.integers(1, 40) * seg + rng.integers(-30, 30), rng.integers(1, 400000)]))
        n = max(n, 1)
        pre, enc = int(rng.integers(0, 2)), int(rng.integers(0, 3))
        g = int(1 << rng.integers(0, 12)) if rng.random() < 0.5 else int(rng.integers(1, 3000))
        outl = int(rng.integers(1, 400))
        scale = 2.0 ** rng.uniform(0, 14)
        v = rng.laplace(0, scale, n)
        if rng.random() < 0.5:
            v = np.cumsum(v) * 0.05
        v = np.clip(np.round(v), -32768, 32767).astype(np.int64)
        if kind == "u16":
            x = (v & 0xFFFF).astype(np.uint16)
        elif kind == "i16":
            x = v.astype(np.int16)
        else:
            x = ((v & 0xFFFF) | (rng.integers(-9, 9, n) << 16)).astype(np.int32)
        yield t, kind, x, pre, enc, g, outl


def test_random_round_trip(eng):
    seen = set()
    bad = []
    for t, kind, x, pre, enc, g, outl in random_cases(120):
        size, data = streams.oracle_stream(x, kind, pre, enc, g, outl)
        assert not api.is_error(size), t
        r, st, out = decode(eng, data, x.size, pre, enc, g, outl)
        if r or st != x.size or not np.array_equal(out, low16(x)):
            bad.append((t, kind, x.size, pre, enc, g, outl, size, r, st))
        seen.add((kind, pre, enc, enc and not g & (g - 1)))
    assert not bad, bad[:5]
    # every encoder, Rice and general g, NONE and DIFF, all three sample kinds
    assert {s[0] for s in seen} == {"u16", "i16", "i16_in_i32"}
    assert {s[1] for s in seen} == {0, 1} and {s[2] for s in seen} == {0, 1, 2}
    assert {s[3] for s in seen if s[2] == 1} == {True, False}


def test_output_does_not_depend_on_bytes_past_the_stream(eng):
    t, kind, x, pre, enc, g, outl = next(c for c in random_cases(120) if c[4] == 1 and c[2].size > 5000)
    size, data = streams.oracle_stream(x, kind, pre, enc, g, outl)
    a = decode(eng, data, x.size, pre, enc, g, outl, tail=0xAB)
    b = decode(eng, data, x.size, pre, enc, g, outl, tail=0x00)
    assert a[0] == b[0] == 0 and a[1] == b[1] == x.size
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[2], low16(x))


# ---------------------------------------------------------------- 3. small shapes
ZERO32 = (1, 1, 32, 0)  # DIFF, GOLOMB_ZERO, g = 32


@pytest.mark.parametrize("n", [1, 2, 31, 32, 33, TILE - 1, TILE, TILE + 1, 2 * TILE + 1])
def test_small_shapes(eng, n):
    assert_round_trip(eng, laplace_u16(11, 2 * TILE + 1)[:n], "u16", *ZERO32, n)


def stream_size(x):
    return streams.oracle_stream(x, "u16", *ZERO32)[0]


def test_around_one_workgroup_span(eng):
    """The largest n whose stream fits one workgroup's span of 16384 bytes and
    the smallest whose stream does not (a stream's size grows with n: the
    stream of a prefix is a prefix of the stream)."""
    x = laplace_u16(12, 40000)
    assert stream_size(x) > WG_SPAN
    lo, hi = 1, x.size  # size(lo) <= span < size(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if stream_size(x[:mid]) <= WG_SPAN:
            lo = mid
        else:
            hi = mid
    assert stream_size(x[:lo]) <= WG_SPAN < stream_size(x[:hi]) and hi == lo + 1
    for n in (lo, hi):
        assert_round_trip(eng, x[:n], "u16", *ZERO32, n)


@pytest.mark.parametrize("n", [5, TILE + 77])
def test_dst_offset_by_two_bytes(eng, n):
    # dst 2 but not 16-byte aligned: the scalar store path
    assert_round_trip(eng, laplace_u16(13, n), "u16", *ZERO32, n, dst_off=2)


# ---------------------------------------------------------------- 4. the carried loops
def test_past_1024_workgroups_and_1024_tiles(eng):
    """More than 1024 parse workgroups and more than 1024 DIFF tiles: the
    second pass of dec_scan_kernel's and dec_tile_prefix_kernel's loops, which
    no frame reaches."""
    n = 7 * (1 << 20) + 4097
    x = np.random.default_rng(7).integers(0, 65536, n, dtype=np.uint16)
    size, data = streams.oracle_stream(x, "u16", 1, 1, 4096, 0)
    assert not api.is_error(size)
    assert size > 1025 * WG_SPAN and n > 1025 * TILE, \
        f"input no longer reaches the second pass of the loops: {size} bytes, {n} samples"
    r, st, out = decode(eng, data, n, 1, 1, 4096, 0)
    assert r == 0 and st == n, (api.error_name(r), api.error_name(st) if api.is_error(st) else st)
    assert np.array_equal(out, x)


def samples_of_48_bits(n):
    """n int16 samples (device) whose DIFF + GOLOMB_MULTI g = 1, outlier 24 codewords all take the
    worst case of 48 bits: residuals r in [8204, 32767], so the mapped value 2r is at least
    24 + 2^14 and escapes at the top level (encoder.c:353-376: 31 ones, a zero, 16 raw bits).
    The raw bits 2r - 24 end in a zero, so a parse begun anywhere falls into step at the next
    codeword and the speculative parse settles at once."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(5)
    r = torch.randint(8204, 32768, (n,), generator=g, device="cuda", dtype=torch.int32)
    return (torch.cumsum(r, 0, dtype=torch.int64) & 0xFFFF).to(torch.int16)  # int16 wrap


def test_stream_of_the_largest_size(eng):
    """CMP_GPU_STREAM_DECODE_MAX bytes exactly, 2^32 - 4096 bits: the last range ends at
    8388600 * 512, the last exit 4096 below the 32-bit wrap; 32768 workgroups, 21846 tiles.
    89478400 samples at 48 bits each, from the GPU encoder."""
    import torch
    pkg = load_pkg()
    n = pkg.STREAM_DECODE_MAX // 6
    assert n == 89478400
    x = samples_of_48_bits(n)
    cap = 6 * n + 64
    enc = torch.full((cap + 64,), 0xAB, dtype=torch.uint8, device="cuda")
    size = torch.zeros(1, dtype=torch.int32, device="cuda")
    assert eng.encode_stream("i16", x.data_ptr(), n, 1, 2, 1, 24, enc.data_ptr(), cap, size.data_ptr()) == 0
    assert eng.synchronize() == 0
    assert int(size.cpu().numpy().astype(np.uint32)[0]) == pkg.STREAM_DECODE_MAX
    dst = torch.full((n + GUARD,), 0xA5A5 - 0x10000, dtype=torch.int16, device="cuda")
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    r = eng.decode_stream(enc.data_ptr(), pkg.STREAM_DECODE_MAX, n, 1, 2, 1, 24, dst.data_ptr(), st.data_ptr())
    assert r == 0, api.error_name(r)
    assert eng.synchronize() == 0
    s = int(st.cpu().numpy().astype(np.uint32)[0])
    assert s == n, api.error_name(s) if api.is_error(s) else s
    assert torch.equal(dst[:n], x)
    assert bool((dst[n:] == 0xA5A5 - 0x10000).all())


# ---------------------------------------------------------------- 5. invalid streams
def zero32_end_bit(x):
    """bit position where the last codeword of the DIFF + GOLOMB_ZERO g = 32
    stream of x ends (encoder.c:335-351: value m + 1 below the outlier 543 as
    q ones, a zero and 5 bits; else the zero codeword and 16 raw bits)"""
    r = np.diff(x.astype(np.int64), prepend=0)
    r = ((r + 32768) & 0xFFFF) - 32768  # int16 wrap
    m = np.where(r >= 0, 2 * r, -2 * r - 1)
    bits = np.where(m < 543, (m + 1) // 32 + 6, 22)
    return int(bits.sum())


@pytest.fixture(scope="module")
def odd_stream():
    """a few thousand samples whose stream ends inside a byte"""
    for n in range(3000, 3064):
        x = laplace_u16(14, 3064)[:n]
        size, data = streams.oracle_stream(x, "u16", *ZERO32)
        e = zero32_end_bit(x)
        assert (e + 7) // 8 == size, (e, size)  # the restated lengths agree with the oracle
        if e % 8:
            return x, data, e
    raise AssertionError("no stream with pad bits found")


def bitstream_error(eng, data, n, args, src_size=None):
    r, st, _ = decode(eng, data, n, *args, src_size=src_size)
    assert r == 0, api.error_name(r)
    assert api.is_error(st) and api.error_name(st) == "INT_BITSTREAM", st


def test_invalid_streams(eng, odd_stream):
    x, data, e = odd_stream
    n, size = x.size, len(data)
    assert e % 8 != 0 and size > 16
    # the stream itself is fine
    r, st, out = decode(eng, data, n, *ZERO32)
    assert (r, st) == (0, n) and np.array_equal(out, x)
    bitstream_error(eng, data, n + 1, ZERO32)
    bitstream_error(eng, data, n - 1, ZERO32)
    bitstream_error(eng, data[:size - 1], n, ZERO32)
    bitstream_error(eng, data[:size - 8], n, ZERO32)
    bitstream_error(eng, data + b"\0\0\0\0", n, ZERO32)
    pad = bytearray(data)
    pad[-1] |= 1  # the last pad bit
    bitstream_error(eng, bytes(pad), n, ZERO32)
    pad = bytearray(data)
    pad[-1] |= 1 << (8 - e % 8 - 1)  # the first pad bit
    assert pad[-1] != data[-1]
    bitstream_error(eng, bytes(pad), n, ZERO32)


def test_uncompressed_needs_two_bytes_per_sample(eng):
    x = laplace_u16(15, 1000)
    size, data = assert_round_trip(eng, x, "u16", 0, 0, 0, 0, "uncompressed")
    assert size == 2 * x.size
    bitstream_error(eng, data + b"\0\0", x.size, (0, 0, 0, 0))
    bitstream_error(eng, data[:-2], x.size, (0, 0, 0, 0))


# ---------------------------------------------------------------- 6. engine reuse
def test_engine_reuse(eng, orc, odd_stream):
    """valid stream, invalid stream, a frame batch, the first stream again on
    one engine: scratch slots and flags carry no state over"""
    import torch
    x = laplace_u16(16, 3 * TILE + 5)
    assert_round_trip(eng, x, "u16", *ZERO32, "first")
    bad_x, bad, _ = odd_stream
    bitstream_error(eng, bad, bad_x.size + 1, ZERO32)
    # three DIFF + GOLOMB_ZERO frames from the oracle's encoder through cmp_gpu_decompress
    p = api.CmpParams(primary_preprocessing=1, primary_encoder_type=1, primary_encoder_param=16)
    xs = [laplace_u16(20 + i, m) for i, m in enumerate((1, 4097, 9001))]
    frames = []
    for f in xs:
        ctx = api.CmpContext()
        assert not api.is_error(orc.initialise(ctx, p))
        cap = 26 + 6 * f.size + 64
        dst = api.aligned_empty(cap)
        r = orc.compress_u16(ctx, dst, cap, f)
        assert not api.is_error(r), api.error_name(r)
        frames.append(bytes(dst[:r]))
    cap = (max(len(f) for f in frames) + 7) // 8 * 8
    host = np.zeros(len(frames) * cap, dtype=np.uint8)
    for i, f in enumerate(frames):
        host[i * cap:i * cap + len(f)] = np.frombuffer(f, dtype=np.uint8)
    src = torch.from_numpy(host).cuda()
    nmax = max(f.size for f in xs)
    out = torch.zeros(len(frames) * nmax, dtype=torch.int16, device="cuda")
    st = torch.zeros(len(frames), dtype=torch.int32, device="cuda")
    assert eng.decompress(src.data_ptr(), cap, cap, len(frames), out.data_ptr(), 2 * nmax, nmax, st.data_ptr()) == 0
    assert eng.synchronize() == 0
    got = out.cpu().numpy().view(np.uint16)
    for i, f in enumerate(xs):
        assert int(st[i]) == f.size, i
        assert np.array_equal(got[i * nmax:i * nmax + f.size], f), i
    assert_round_trip(eng, x, "u16", *ZERO32, "again")
