"""Shared pieces of the Rice/ZERO frame kernel's GPU tests (test_gpu_rice.py,
test_gpu_rice_lookback.py, test_gpu_stream.py): the device layer's launch
counters, sample generators, the oracle and GPU runners and the mismatch
report."""
import ctypes
import functools
import zlib

import numpy as np

from conftest import load_pkg

api = load_pkg().cmpapi
P = api.CmpParams
SEG = 16384  # samples per segment of the Rice kernel
HDR = 22     # bytes of a GOLOMB_ZERO frame header

# airs_dev.h enum airs_launch_stat
LB1, LB0, RICE_STREAM, RICE_AUTO, ENCODE, ENCODE_STREAM, DECODE_ROUND, WALK_CTX, WALK_SEG, FB_STEP = range(10)
STAT_NAMES = ("rice_lb1", "rice_lb0", "rice_stream", "rice_auto", "encode", "encode_stream", "decode_round",
              "walk_ctx", "walk_seg", "fb_step")


def launch_stats(prod):
    """The process-wide host-side launch counters of the loaded libairscmp.so
    (airs_dev_launch_stats), as a list of ints."""
    fn = prod.lib.airs_dev_launch_stats
    fn.argtypes = [ctypes.POINTER(ctypes.c_uint64), ctypes.c_uint32]
    fn.restype = ctypes.c_uint32
    out = (ctypes.c_uint64 * len(STAT_NAMES))()
    assert fn(out, len(STAT_NAMES)) == len(STAT_NAMES)
    return [int(v) for v in out]


class Launches:
    """with Launches(prod) as l: ...; l.delta is the counters' increase, and
    l.only(LB1) asserts that the launches of the block were of that one kind
    (count: exactly that many; None: at least one).  fb_step is not a kind of
    encode launch: the device state machine's step runs beside the encode
    launches of a batch below the worst-case capacity, and only() leaves it
    to the tests that ask for it."""

    def __init__(self, prod):
        self.prod = prod

    def __enter__(self):
        self.before = launch_stats(self.prod)
        self.delta = None
        return self

    def __exit__(self, *exc):
        self.delta = [a - b for a, b in zip(launch_stats(self.prod), self.before)]
        return False

    def named(self):
        return {n: d for n, d in zip(STAT_NAMES, self.delta) if d}

    def only(self, which, count=None):
        d = self.delta
        assert d[which] >= 1 and all(v == 0 for i, v in enumerate(d) if i not in (which, FB_STEP)), self.named()
        if count is not None:
            assert d[which] == count, self.named()


def frame(rng, kind, n, k, data):
    if data == "laplace":
        x = np.round(rng.laplace(0, 2.0 ** k, n)).astype(np.int64)
        x = np.cumsum(x) if rng.random() < 0.5 else x
    elif data == "outliers":
        x = np.round(rng.laplace(0, 2.0 ** k, n)).astype(np.int64) + 16384
        idx = rng.integers(0, n, max(1, n // 700))
        x[idx] = rng.integers(0, 65536, idx.size)
        x[::4099] = 0x8000 + x[::4099]  # an outlier at every alignment
    elif data == "uniform":
        x = rng.integers(0, 65536, n)
    elif data == "const":
        x = np.full(n, int(rng.integers(0, 65536)), dtype=np.int64)
    else:  # extreme: the largest mapped value, NONE and DIFF
        x = np.where(np.arange(n) % 2 == 0, 32767, -32768).astype(np.int64)
        x[rng.integers(0, n, 50)] = 0
    return as_kind(x, kind)


def as_kind(x, kind):
    x = np.asarray(x).astype(np.int64) & 0xFFFF
    return x.astype(np.uint16) if kind == "u16" else x.astype(np.uint16).view(np.int16)


POOL = 1 << 22  # samples per pool


@functools.lru_cache(maxsize=4)
def pool(k, data):
    """One pool of 16-bit patterns per (k, data kind), frames and segments are
    slices of it: laplace (scale 2^k), outliers (laplace around 16384 with
    single-sample outliers), uniform."""
    rng = np.random.default_rng(zlib.crc32(f"pool/{k}/{data}".encode()))
    if data == "uniform":
        x = rng.integers(0, 65536, POOL)
    else:
        x = np.round(rng.laplace(0, 2.0 ** k, POOL)).astype(np.int64)
        if data == "outliers":
            x += 16384
            idx = rng.integers(0, POOL, POOL // 700)
            x[idx] = rng.integers(0, 65536, idx.size)
            x[::4099] = 0x8000 + x[::4099]
    x = (x & 0xFFFF).astype(np.uint16)
    x.setflags(write=False)
    return x


def pool_frames(rng, kind, nf, spf, k, data):
    """nf frames of spf segments.  laplace, outliers, uniform: a slice of the
    pool per frame.  mixed: every segment of a frame is, independently, a
    constant, laplace noise at scale 2^k or uniform noise (seeded proportions,
    all three in every frame; spf >= 3): segments of very different coding
    time and size side by side, the uniform ones too large for the arena."""
    n = spf * SEG
    frames = []
    if data != "mixed":
        src = pool(k, data)
        for off in rng.integers(0, POOL - n, nf):
            frames.append(src[off:off + n])
    else:
        lap, uni = pool(k, "laplace"), pool(k, "uniform")
        p = rng.dirichlet((4.0, 4.0, 4.0))
        for _ in range(nf):
            kinds = rng.choice(3, spf, p=p)
            kinds[rng.permutation(spf)[:3]] = (0, 1, 2)
            x = np.empty(n, dtype=np.uint16)
            offs = rng.integers(0, POOL - SEG, spf)
            consts = rng.integers(0, 65536, spf)
            for s in range(spf):
                seg = x[s * SEG:(s + 1) * SEG]
                if kinds[s] == 0:
                    seg[:] = consts[s]
                else:
                    seg[:] = (lap if kinds[s] == 1 else uni)[offs[s]:offs[s] + SEG]
            frames.append(x)
    return [f if kind == "u16" else f.view(np.int16) for f in frames]


def params(pre, g, checksum):
    return P(primary_preprocessing=pre, primary_encoder_type=api.ENCODER_GOLOMB_ZERO, primary_encoder_param=g,
             checksum_enabled=checksum)


def oracle_at(orc, kind, pre, g, x, checksum, cap=None):
    """The oracle's compress of one frame on a fresh context at capacity cap
    (default: the bound): (return value, the frame's bytes or None on error)."""
    ctx = api.CmpContext()
    assert not api.is_error(orc.initialise(ctx, params(pre, g, checksum)))
    cap = orc.compress_bound(2 * x.size) if cap is None else cap
    dst = api.aligned_empty(max(cap, 8))
    r = orc.compress(kind, ctx, dst, cap, x)
    return r, (None if api.is_error(r) else bytes(dst[:r]))


def oracle(orc, kind, pre, g, frames, checksum):
    want = []
    for x in frames:
        r, b = oracle_at(orc, kind, pre, g, x, checksum)
        assert b is not None, api.error_name(r)
        want.append(b)
    return want


def gpu_raw(prod, eng, kind, pre, g, frames, checksum, cap=None, dst_stride=None, src_stride=None, src_offset=0,
            ctx_per_frame=False):
    """One cmp_gpu_compress call over the frames (one context and len(frames)
    frames per context, or one context per frame), destinations pre-filled
    with 0xAB: (sizes as uint32, the destination rows [nf, dst_stride])."""
    import torch
    n, nf = frames[0].size, len(frames)
    stride = 2 * n if src_stride is None else src_stride
    host = np.zeros(src_offset + nf * stride + 16, dtype=np.uint8)
    for f, x in enumerate(frames):
        host[src_offset + f * stride:src_offset + f * stride + 2 * n] = np.ascontiguousarray(x).view(np.uint8)
    src = torch.from_numpy(host).cuda()
    cap = prod.compress_bound(2 * n) if cap is None else cap
    dstride = (cap + 7) // 8 * 8 if dst_stride is None else dst_stride
    dst = torch.full((nf * dstride,), 0xAB, dtype=torch.uint8, device="cuda")
    sizes = torch.zeros(nf, dtype=torch.int32, device="cuda")
    ctxs = (api.CmpContext * (nf if ctx_per_frame else 1))()
    for c in ctxs:
        assert not api.is_error(prod.initialise(c, params(pre, g, checksum)))
    torch.cuda.synchronize()
    r = eng.compress(ctxs, 1 if ctx_per_frame else nf, kind, src.data_ptr() + src_offset, stride, 2 * n,
                     dst.data_ptr(), dstride, cap, sizes.data_ptr(), 0)
    assert r == 0, api.error_name(r)
    assert eng.synchronize() == 0
    return sizes.cpu().numpy().astype(np.uint32), dst.cpu().numpy().reshape(nf, dstride)


def gpu(prod, eng, kind, pre, g, frames, checksum, **kw):
    sz, out = gpu_raw(prod, eng, kind, pre, g, frames, checksum, **kw)
    got = []
    for f in range(len(frames)):
        assert not api.is_error(int(sz[f])), (f, api.error_name(int(sz[f])))
        got.append(out[f, :int(sz[f])].tobytes())
    return got


def mask(b):
    """Header bytes 8-13: the clock-derived identifier."""
    b = bytearray(b)
    b[8:14] = b"\0" * 6
    return bytes(b)


def first_diff(a, b):
    """Index of the first differing byte of two byte strings (the shorter
    length when one is a prefix of the other), or None."""
    m = min(len(a), len(b))
    if a[:m] != b[:m]:
        d = np.frombuffer(a, np.uint8, m) != np.frombuffer(b, np.uint8, m)
        return int(np.argmax(d))
    return None if len(a) == len(b) else m


def segment_of_byte(orc, kind, pre, g, x, byte):
    """The segment of frame x whose bits reach frame byte `byte`, from the
    oracle's sizes of the frame's prefixes of whole segments (payload bits
    up to segment s end in byte size(x[:(s + 1) SEG]) - 1); the segment count
    for a byte behind the payload (checksum)."""
    spf = x.size // SEG
    for s in range(spf):
        r, _ = oracle_at(orc, kind, pre, g, x[:(s + 1) * SEG], 0)
        if not api.is_error(r) and byte < r:
            return s
    return spf


def compare(orc, kind, pre, g, frames, got, want, note=""):
    """Assert the frames bit-exact (identifier masked); the failure names every
    differing frame, and for the first one its sizes (a wrong size shows in
    the header first), its first differing byte behind the header, the two
    byte values and that byte's segment."""
    bad = [f for f in range(len(frames)) if mask(got[f]) != mask(want[f])]
    if not bad:
        return
    f = bad[0]
    hb = first_diff(mask(got[f])[:HDR], mask(want[f])[:HDR])
    b = first_diff(got[f][HDR:], want[f][HDR:])
    where = "payload equal"
    if b is not None:
        b += HDR
        gb = got[f][b] if b < len(got[f]) else None
        wb = want[f][b] if b < len(want[f]) else None
        seg = segment_of_byte(orc, kind, pre, g, frames[f], b)
        where = f"first differing payload byte {b} (got {gb}, want {wb}) in segment {seg} of {frames[f].size // SEG}"
    raise AssertionError(f"{note}: frames {bad} differ; frame {f}: sizes got {len(got[f])} want {len(want[f])}, "
                         f"first differing header byte {hb}, {where}")
