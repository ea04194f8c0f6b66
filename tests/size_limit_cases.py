"""The cases of test_size_cases.py (CPU: the oracle against the reference and
the recorded digests) and test_gpu_size_limits.py (GPU: the library against
the oracle): batches whose frames land exactly on a limit, built with
size_cases.py.

A case is what batch_scenarios.run_batch_host / run_batch_gpu take (params,
kind, n, nctx, fpc, cap, srcs) plus `want`, the size each built frame must
have at full capacity without the fallback (frame index -> size or error
value); self_check() asserts it on the oracle, so a case that misses its limit
stops the test.  Cases are built once per process (cached by name).

  capacity   nine frames of sizes S-4 .. S+4 (eight: S-3 .. S+4) at capacity
             S, one context per frame, S mod 8 and the checksum given
  fallback   DIFF + ZERO g=16, then MODEL + MULTI g=8 o=107 rate 11: one
             context per compressed size raw-2 .. raw+2, once as the primary
             pass, once as the secondary pass of acquisition 2 of 5
  failbit    MODEL passes without the fallback at a capacity below the frame:
             the sample that ends on bit 64 (cap / 8) + 63 keeps its new model,
             the one that ends a bit later is the first that does not
  size24     frames of 0xFFFFFE, 0xFFFFFF and 0x1000000 bytes
  fb24       fallback frames of 16 777 214 and 16 777 216 bytes
"""
import copy
import zlib

import numpy as np

import size_cases as sc
from conftest import load_pkg

api = load_pkg().cmpapi
P = api.CmpParams
SEG = 16384
TOO_LARGE = api.err_value("HDR_CMP_SIZE_TOO_LARGE")
TOO_SMALL = api.err_value("DST_TOO_SMALL")

_CACHE = {}


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


class Case:
    def __init__(self, name, params, kind, n, nctx, fpc, cap, srcs, want, auto_k=None, first_lost=None, splits=None):
        self.name, self.params, self.kind, self.n = name, params, kind, n
        self.nctx, self.fpc, self.cap, self.srcs, self.want = nctx, fpc, cap, srcs, want
        self.splits = splits          # acquisitions per cmp_gpu_compress call (default: one call)
        self.auto_k = auto_k          # CMP_GPU_AUTO_RICE: the k every frame must select
        self.first_lost = first_lost  # failbit: context -> (frame, first sample that keeps its old model)

    def batch(self):
        return self.params, self.kind, self.n, self.nctx, self.fpc, self.cap, self.srcs


def cached(fn):
    def wrapped(orc, *key):
        k = (fn.__name__,) + key
        if k not in _CACHE:
            _CACHE[k] = fn(orc, *key)
        return _CACHE[k]
    return wrapped


def select_g(orc_ext, kind, pre):
    """src -> g of CMP_GPU_AUTO_RICE (the oracle's orc_select_rice_k), the
    primary_g hook of run_batch_host."""
    def primary_g(x):
        x = np.ascontiguousarray(x)
        return 1 << orc_ext.orc_select_rice_k(x.ctypes.data, x.size, 1 if kind == "i16_in_i32" else 0, pre, None)
    return primary_g


def self_check(orc, case, orc_ext=None):
    """Every built frame has its intended size on the oracle at full capacity
    (fallback off); AUTO frames select the intended k; failbit frames lose
    their model from the intended sample on at the case's capacity."""
    pcs = list(case.params) if isinstance(case.params, (list, tuple)) else [case.params] * case.nctx
    hook = None
    if case.auto_k is not None:
        hook = select_g(orc_ext, case.kind, pcs[0].primary_preprocessing)
    for c in range(case.nctx):
        idx = [f - c * case.fpc for f in case.want if f // case.fpc == c]
        if not idx:
            continue
        p = copy.copy(pcs[c])
        p.uncompressed_fallback_enabled = 0
        frames = case.srcs[c * case.fpc:c * case.fpc + max(idx) + 1]
        got = sc.replay(orc, api, case.kind, p, frames, primary_g=hook)
        for a in idx:
            assert got[a][0] == case.want[c * case.fpc + a], (case.name, c, a, got[a][0], case.want[c * case.fpc + a])
        if hook is not None:
            assert all(hook(f) == 1 << case.auto_k for f in frames), case.name
        if case.first_lost:
            a, lost = case.first_lost[c]
            frames = case.srcs[c * case.fpc:c * case.fpc + a + 1]
            got = sc.replay(orc, api, case.kind, p, frames, cap=case.cap)
            before, (r, after) = got[a - 1][1], got[a]
            assert r == TOO_SMALL, (case.name, c, api.error_name(r))
            assert after[lost - 1] != before[lost - 1] and (after[lost:] == before[lost:]).all(), (case.name, c)
            assert after[lost] != sc.replay(orc, api, case.kind, p, frames)[a][1][lost], (case.name, c)


# ---- capacity ---------------------------------------------------------------

CODERS = {  # name: (enc, g, outlier)
    "zero3": (sc.ZERO, 3, 0), "zero256": (sc.ZERO, 256, 0), "multi8": (sc.MULTI, 8, 107),
}


def _family(name, enc, g, outl, n, auto_k=None):
    """The base frame of a coder and length (size_cases.Family), shared by the
    capacity cases of every residue and checksum setting."""
    key = ("family", name, enc, g, outl, n, auto_k)
    if key not in _CACHE:
        t = sc.length_table(enc, g, outl)
        lo, hi = sc.run_of_lengths(t)
        if auto_k is None:
            _CACHE[key] = sc.Family(enc, g, outl, n, n * (lo + hi) // 2, _rng(name))
        else:  # lengths k+2 and k+3 only: 2^k codes them in the fewest bits, ties go to the smaller k
            _CACHE[key] = sc.Family(enc, g, outl, n, n * (auto_k + 2) + n // 2, _rng(name), jitter=0.0,
                                    lo=auto_k + 2, hi=auto_k + 3)
    return _CACHE[key]


@cached
def capacity(orc, family, kind, pre, enc, g, outl, n, nctx, res, ck, auto_k=None):
    """nctx frames (9: S-4 .. S+4; 8: S-3 .. S+4) at capacity S, S mod 8 = res."""
    name = f"cap/{family}/{kind}/p{pre}e{enc}g{g}/n{n}/r{res}/ck{ck}"
    rng = _rng(name)
    fam = _family(f"cap/{family}/e{enc}g{g}/n{n}", enc, g, outl, n, auto_k)
    S = sc.frame_size(fam.bits, pre, enc, ck)
    S += (res - S) % 8
    offs = range(-4, 5) if nctx == 9 else range(-3, 5)
    srcs, want = [], {}
    for i, d in enumerate(offs):
        pad = (3 * i + res) % 8  # payload bit counts that are whole bytes, and that are not
        srcs.append(fam.frame(kind, pre, sc.payload_bits(S + d, pre, enc, ck, pad), rng))
        want[i] = S + d
    p = P(primary_preprocessing=pre, primary_encoder_type=enc, primary_encoder_param=7 if auto_k is not None else g,
          primary_encoder_outlier=outl, checksum_enabled=ck)
    return Case(name, p, kind, n, nctx, 1, S, srcs, want, auto_k=auto_k)


@cached
def capacity_raw(orc, kind, n, d, ck):
    """UNCOMPRESSED frames have one size R: two frames at capacity R + d."""
    name = f"cap/raw/{kind}/n{n}/d{d}/ck{ck}"
    rng = _rng(f"cap/raw/{kind}/n{n}")
    srcs = [sc.samples(kind, sc.NONE, rng.integers(0, 65536, n), rng) for _ in range(2)]
    R = sc.raw_size(n, ck)
    p = P(primary_preprocessing=0, primary_encoder_type=0, checksum_enabled=ck)
    return Case(name, p, kind, n, 2, 1, R + d, srcs, {0: R, 1: R})


# ---- fallback ---------------------------------------------------------------

FB = dict(primary_preprocessing=1, primary_encoder_type=1, primary_encoder_param=16, secondary_iterations=15,
          secondary_preprocessing=3, secondary_encoder_type=2, secondary_encoder_param=8,
          secondary_encoder_outlier=107, model_rate=11)
FB_OFFS = (-2, -1, 0, 1, 2)
FB_FPC, FB_MID = 5, 2


def _near(x, kind, rng, amp=4):
    """x plus small noise: a frame that compresses against a model near x."""
    return sc.from_low16(kind, sc.low16(x).astype(np.int64) + rng.integers(-amp, amp + 1, len(x)), rng)


@cached
def fallback(orc, kind, n, ck, worst, reps=1):
    """Ten contexts (times reps): context 2i has its first frame (primary
    pass) at raw + FB_OFFS[i] bytes compressed, context 2i+1 its frame of
    acquisition FB_MID (secondary pass).  The frames before the edge are a
    random walk plus noise, the frames after it the edge frame plus noise, so
    they compress against the model whichever way the edge went, and carry the
    sequence number and identifier the decision leaves.  cap: the raw frame
    size, or (worst) the worst case."""
    name = f"fb/{kind}/n{n}/ck{ck}"
    rng = _rng(name)
    raw = sc.raw_size(n, ck)
    p = P(**FB, checksum_enabled=ck, uncompressed_fallback_enabled=1)
    q = P(**FB, checksum_enabled=ck)
    key = ("fbctx", name)
    if key not in _CACHE:
        ctxs, want = [], {}
        for i, d in enumerate(FB_OFFS):
            pad = (3 * i) % 8
            # the edge as the primary pass
            f0 = sc.sized_frame(kind, sc.DIFF, sc.ZERO, 16, 0, n, raw + d, ck, rng, pad)
            ctxs.append([f0] + [_near(f0, kind, rng) for _ in range(FB_FPC - 1)])
            want[(2 * i, 0)] = raw + d
            # the edge as a secondary pass
            walk = sc.samples(kind, sc.DIFF, rng.integers(0, 8, n), rng)
            pre = [_near(walk, kind, rng) for _ in range(FB_MID)]
            model = sc.replay(orc, api, kind, q, pre)[-1][1]
            fm = sc.sized_frame(kind, sc.MODEL, sc.MULTI, 8, 107, n, raw + d, ck, rng, (pad + 4) % 8, model=model)
            ctxs.append(pre + [fm] + [_near(fm, kind, rng) for _ in range(FB_FPC - FB_MID - 1)])
            want[(2 * i + 1, FB_MID)] = raw + d
        _CACHE[key] = ctxs, want
    ctxs, want = _CACHE[key]
    nctx = 10 * reps
    srcs = [f for c in range(nctx) for f in ctxs[c % 10]]
    w = {c * FB_FPC + a: s for (c, a), s in want.items()}
    return Case(name + f"/worst{int(worst)}/x{reps}", p, kind, n, nctx, FB_FPC, 26 + 6 * n if worst else raw, srcs, w)


def fallback_edges(case, frames):
    """From the oracle's frames of a fallback case: {(offset, pass kind):
    'compressed' or 'raw'} of the edge frames of the first ten contexts, each
    checked to be the frame the case means (its size, its pass in the header)."""
    out = {}
    raw = sc.raw_size(case.n, case.params.checksum_enabled)
    for i, d in enumerate(FB_OFFS):
        for sec in (0, 1):
            f = (2 * i + sec) * FB_FPC + (FB_MID if sec else 0)
            r, b = frames[f]
            assert b is not None, (case.name, f, api.error_name(r))
            h = api.parse_header(b)
            if h["encoder_type"] == api.ENCODER_UNCOMPRESSED:
                assert r == raw and h["preprocessing"] == 0 and h["sequence_number"] == 0
                out[(d, sec)] = "raw"
            else:
                assert r == raw + d and h["sequence_number"] == (FB_MID if sec else 0)
                assert (h["preprocessing"], h["encoder_type"]) == ((3, 2) if sec else (1, 1))
                out[(d, sec)] = "compressed"
    return out


# ---- model fail bit ---------------------------------------------------------

FAIL_VARIANTS = ("keep", "lost", "escape")


@cached
def failbit(orc, kind, n, res, ck):
    """Three contexts of three frames at a capacity with cap mod 8 = res, about
    a byte per sample.  Frame 0 (primary pass) fits.  Frame 1 (MODEL + MULTI
    g=8 o=107) does not; with W = cap / 8 and j its sample of the variant:
      keep    sample j-1 ends on bit 64W + 63 of the frame (it keeps its new
              model), sample j is the first that does not
      lost    sample j ends on bit 64W + 64
      escape  sample j is an escape whose first piece ends on bit 64W + 62 and
              whose second piece (2 bits) ends on bit 64W + 64
    (bit positions count the frame's bits from 1: `ends on bit b` = b bits of
    the frame are written after the sample).  Frame 2 is a second MODEL pass
    near the model frame 1 left behind, small enough to fit."""
    name = f"failbit/{kind}/n{n}/r{res}/ck{ck}"
    rng = _rng(name)
    p = P(**FB, checksum_enabled=ck)
    cap = sc.HDR_EXT + n
    cap += (res - cap) % 8
    W = cap // 8
    t = sc.length_table(sc.MULTI, 8, 107)
    srcs, want, lost = [], {}, {}
    for c, variant in enumerate(FAIL_VARIANTS):
        size0 = sc.HDR_EXT + (7 * n) // 8 + c + (4 if ck else 0)
        f0 = sc.sized_frame(kind, sc.DIFF, sc.ZERO, 16, 0, n, size0, ck, rng, pad=c)
        if variant == "keep":
            last, prefix = 9, 64 * W + 63 - 9
        elif variant == "lost":
            last, prefix = 9, 64 * W + 64 - 9 - 9
        else:
            first, second = sc.escape_pieces(sc.MULTI, 8, 107, 107 + 2)
            assert (first, second) == (17, 2)
            last, prefix = None, 64 * W + 62 - first - 9
        prefix -= 8 * sc.HDR_EXT  # payload bits in front of the two samples around the limit
        j = prefix // 12
        head = sc.mapped_with(t, sc.spread(t, j, prefix, rng), rng)
        nine = sc.mapped_with(t, np.array([9, 9]), rng)  # |residual| >= 20: the model visibly moves
        edge = [nine[0], nine[1]] if last else [nine[0], 107 + 2]
        tail = sc.mapped_with(t, sc.spread(t, n - j - 2, 12 * (n - j - 2) + c, rng), rng)
        m = np.concatenate([head, edge, tail])
        f1 = sc.samples(kind, sc.MODEL, m, rng, model=sc.low16(f0))
        # keep: head + nine[0] end on 64W+63, nine[1] (sample j+1) is lost;
        # lost / escape: sample j+1 is the one that ends on 64W+64
        first_lost = j + 1
        got = sc.replay(orc, api, kind, p, [f0, f1], cap=cap)
        f2 = sc.sized_frame(kind, sc.MODEL, sc.MULTI, 8, 107, n, sc.HDR_EXT + (6 * n) // 8 + (4 if ck else 0), ck,
                            rng, pad=3, model=got[1][1])
        srcs += [f0, f1, f2]
        bits1 = int(t[m].sum())
        want[3 * c] = size0
        want[3 * c + 1] = sc.frame_size(bits1, sc.MODEL, sc.MULTI, ck)
        lost[c] = (1, first_lost)
    return Case(name, p, kind, n, 3, 3, cap, srcs, want, first_lost=lost)


# ---- the 24-bit size field --------------------------------------------------

SIZES24 = (0xFFFFFE, 0xFFFFFF, 0x1000000)


@cached
def size24(orc, family):
    """One context, three frames of 0xFFFFFE, 0xFFFFFF and 0x1000000 bytes
    (NONE + ZERO g=1, 2 .. 17 bits per sample): rice: n = 511 x 16384 (whole
    segments: the Rice kernel); encode: n = 8 388 000 (encode_kernel)."""
    n = {"rice": 511 * SEG, "encode": 8388000}[family]
    name = f"size24/{family}"
    rng = _rng(name)
    fam = sc.Family(sc.ZERO, 1, 0, n, sc.payload_bits(SIZES24[1], sc.NONE, sc.ZERO, 0, 3), rng)
    srcs = [fam.frame("u16", sc.NONE, sc.payload_bits(s, sc.NONE, sc.ZERO, 0, pad), rng)
            for s, pad in zip(SIZES24, (0, 3, 5))]
    p = P(primary_preprocessing=0, primary_encoder_type=1, primary_encoder_param=1)
    return Case(name, p, "u16", n, 1, 3, 26 + 6 * n, srcs, {0: SIZES24[0], 1: SIZES24[1], 2: TOO_LARGE})


@cached
def size24_calls(orc):
    """One context with secondary passes, one frame per cmp_gpu_compress call:
    a frame of 0x1000000 bytes (HDR_CMP_SIZE_TOO_LARGE: the context stays at
    its primary pass), then two small frames: a primary and a secondary pass."""
    n = 8388000
    rng = _rng("size24/calls")
    big = sc.sized_frame("u16", sc.NONE, sc.ZERO, 1, 0, n, SIZES24[2], 0, rng, 1)
    small = [rng.integers(0, 4, n).astype(np.uint16) for _ in range(2)]
    p = P(primary_preprocessing=0, primary_encoder_type=1, primary_encoder_param=1, secondary_iterations=2,
          secondary_preprocessing=1, secondary_encoder_type=1, secondary_encoder_param=1)
    return Case("size24/calls", p, "u16", n, 1, 3, 26 + 6 * n, [big] + small, {0: TOO_LARGE}, splits=[1, 1, 1])


@cached
def fb24(orc, n):
    """One fallback context with secondary passes: a noise frame (falls back;
    n = 8 388 599: a raw frame of 16 777 214 bytes is written; n = 8 388 600:
    16 777 216 bytes, HDR_CMP_SIZE_TOO_LARGE), a quiet frame, and the quiet
    frame plus noise: the pass of each depends on how the one before ended."""
    name = f"fb24/n{n}"
    rng = _rng(name)
    noise = rng.integers(0, 65536, n).astype(np.uint16)
    quiet = (np.cumsum(rng.integers(-3, 4, n)) & 0xFFFF).astype(np.uint16)
    srcs = [noise, quiet, _near(quiet, "u16", rng)]
    p = P(**FB, uncompressed_fallback_enabled=1)
    return Case(name, p, "u16", n, 1, 3, 26 + 6 * n, srcs, {})


# ---- payload-only streams ---------------------------------------------------

@cached
def stream(orc, which, res):
    """(x, kind, pre, enc, g, outlier, size): a stream of exactly `size`
    bytes, size mod 8 = res.  rice: u16, DIFF + ZERO g=4, two whole segments
    (the Rice kernel's stream launch); encode: i16_in_i32, NONE + MULTI g=8
    o=107, 8192 + 1 samples (encode_kernel's)."""
    kind, pre, enc, g, outl, n = {"rice": ("u16", 1, sc.ZERO, 4, 0, 2 * SEG),
                                  "encode": ("i16_in_i32", 0, sc.MULTI, 8, 107, 8193)}[which]
    rng = _rng(f"stream/{which}/{res}")
    t = sc.length_table(enc, g, outl)
    lo, hi = sc.run_of_lengths(t)
    size = n * (lo + hi) // 16
    size += (res - size) % 8
    bits = 8 * size - (res % 8 and 3)
    x = sc.samples(kind, pre, sc.mapped_with(t, sc.spread(t, n, bits, rng), rng), rng)
    return x, kind, pre, enc, g, outl, size


# ---- the catalogue ----------------------------------------------------------

def cpu_catalogue(orc):
    """name -> case: every case of the GPU tests at the size the CPU tests run
    (the context walk's 128 contexts are its ten distinct ones, repeated)."""
    out = []
    for res in range(8):
        for ck in (0, 1):
            for k in (0, 5):
                out.append(capacity(orc, "rice_lb0", ("u16", "i16")[k & 1], k & 1, sc.ZERO, 1 << k, 0, 2 * SEG, 9,
                                    res, ck))
            k, pre = ((3, 1), (5, 0))[res & 1]
            out.append(capacity(orc, "rice_lb1", ("u16", "i16")[res & 1], pre, sc.ZERO, 1 << k, 0, 17 * SEG, 8,
                                res, ck))
            for n in (4160, 16385):
                for kind in ("u16", "i16_in_i32"):
                    for cname, (enc, g, outl) in CODERS.items():
                        out.append(capacity(orc, "encode", kind, (res + ck) & 1, enc, g, outl, n, 9, res, ck))
            out.append(capacity(orc, "auto", "i16_in_i32", res & 1, sc.ZERO, 1 << 3, 0, 16385, 9, res, ck, 3))
            out.append(capacity(orc, "auto", "u16", res & 1, sc.ZERO, 1 << 5, 0, 4160, 9, res, ck, 5))
    for ck in (0, 1):
        for d in range(-4, 5):
            for n, kind in ((4160, "u16"), (16385, "i16_in_i32")):
                out.append(capacity_raw(orc, kind, n, d, ck))
    for ck in (0, 1):
        for worst in (False, True):
            out.append(fallback(orc, ("u16", "i16_in_i32")[ck], 8192, ck, worst))
            out.append(fallback(orc, ("i16_in_i32", "u16")[ck], 65536, ck, worst))
    for res in (0, 1, 7):
        out.append(failbit(orc, ("u16", "i16_in_i32", "i16")[res % 3], 12288, res, res & 1))
    out += [size24(orc, "rice"), size24(orc, "encode"), size24_calls(orc), fb24(orc, 8388599), fb24(orc, 8388600)]
    return {c.name: c for c in out}


def trace(lib, case, orc_ext=None):
    """The case's call loop (c-major) on any CmpLib, observed after every
    call: (return value, sha256 of the frame's bytes, the context's
    identifier, sequence number and model size, sha256 of its work buffer)."""
    import hashlib

    import batch_scenarios as bs
    sb = 4 if case.kind == "i16_in_i32" else 2
    pcs = list(case.params) if isinstance(case.params, (list, tuple)) else [case.params] * case.nctx
    hook = select_g(orc_ext, case.kind, pcs[0].primary_preprocessing) if case.auto_k is not None else None
    lib.set_timestamp_func(bs._ts_counter(5000))
    try:
        out = []
        dst = api.aligned_empty(case.cap + 64)
        for c in range(case.nctx):
            w = lib.cal_work_buf_size(pcs[c], case.n * sb)
            assert not api.is_error(w)
            buf = api.aligned_empty(max(w, 2), fill=0)
            ctx = api.CmpContext()
            r = lib.initialise(ctx, pcs[c], buf if w else None, w)
            assert not api.is_error(r), api.error_name(r)
            for a in range(case.fpc):
                x = case.srcs[c * case.fpc + a]
                if hook is not None:
                    ctx.params.primary_encoder_param = hook(x)
                dst[:] = 0xAB
                r = lib.compress(case.kind, ctx, dst, case.cap, x)
                frame = bytes(dst[:r]) if not api.is_error(r) else b""
                assert bytes(dst[case.cap:]) == b"\xAB" * 64, (case.name, c, a)
                out.append((r, hashlib.sha256(frame).hexdigest(), ctx.identifier, ctx.sequence_number,
                            ctx.model_size, hashlib.sha256(bytes(buf[:w])).hexdigest()))
        return out
    finally:
        lib.set_timestamp_func(None)


def trace_digest(tr):
    import hashlib
    return hashlib.sha256(repr(tr).encode()).hexdigest()
