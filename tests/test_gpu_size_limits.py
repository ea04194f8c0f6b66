"""Frames whose size lands exactly on a limit, through every encode route.

Every route ends in a comparison of a frame's size with a limit, each with its
own copy of the decision.  The cases (size_limit_cases.py, built from
code-length arithmetic by size_cases.py and pinned to the reference by
test_size_cases.py) put frames on the limit and a byte or a bit either side:

  decision (site)                                          test here
  size > cap, Rice kernel (enc_rice.hip rice_kernel
    epilogue, stream and frame)                            test_capacity_rice_lb0 / _lb1, test_capacity_stream[rice]
  store range cap & ~3, tail bytes and checksum < cap
    (enc_rice.hip)                                         test_capacity_rice_* (0xAB fill behind cap; checksum on)
  the same for encode_kernel (enc_kernel.h epilogue)       test_capacity_encode, test_capacity_uncompressed,
                                                           test_capacity_auto, test_capacity_stream[encode]
  bpos <= a.fail_bit (enc_kernel.h)                        test_model_fail_bit[stepwise, flags0]
  size > cap, size > 0xFFFFFF (enc_walk.hip epilogues)     test_fallback_segment_walk, test_fallback_context_walk
  a.fb && size > a.raw_size (enc_walk.hip, context walk)   test_fallback_context_walk
  raw-frame store range raw_size & ~3 (enc_walk.hip)       test_fallback_context_walk (checksum off and on)
  fb_step_kernel: v == err_small, raw_size > 0xFFFFFF
    (encode.hip)                                           test_fallback_routes[stepwise], test_fallback_24bit[stepwise]
  model_fail_bit = 64 (cap / 8) + 63 (cmp_host.c)          test_model_fail_bit (every route)
  fb_eligible, walk eligibility from raw (cmp_batch.c)     test_fallback_routes, test_fallback_24bit[flags0]
  size > 0xFFFFFF, Rice kernel and encode_kernel           test_size_field_24bit

Expectations always come from the oracle's call loop
(batch_scenarios.run_batch_host), never from the library under test, and
everything the batch helpers return is compared: frame bytes with identifiers
unmasked, sizes or error values, each context's identifier, sequence number
and model size, and the work buffers.  Every destination row must also still
hold its 0xAB fill from the capacity to the row's end, for frames that fit
and frames that do not.  Which kernel family or batch route a call took is
asserted from the device layer's host-side counters (airs_dev_launch_stats),
so a case that quietly takes another route fails.
"""
import pytest

import batch_scenarios as bs
import size_cases as sc
import size_limit_cases as lc
import streams
from conftest import load_pkg
from rice_helpers import (ENCODE, ENCODE_STREAM, FB_STEP, LB0, LB1, RICE_STREAM, SEG, WALK_CTX, WALK_SEG, Launches,
                          first_diff)
from test_gpu_stream import gpu_stream

pytestmark = pytest.mark.gpu
pkg = load_pkg()
api = pkg.cmpapi

ROUTES = {"host": None, "host_stepped": api.GPU_HOST_STEPPED, "stepwise": api.GPU_STEPWISE, "flags0": 0}
_WANT = {}


@pytest.fixture(scope="module")
def eng(prod):
    if not prod.gpu_available():
        pytest.fail("GPU test run without a usable HIP device")
    e = prod.engine()
    yield e
    e.close()


def _want(orc, orc_ext, case):
    """The oracle's call loop of the case (once per process)."""
    if case.name not in _WANT:
        hook = lc.select_g(orc_ext, case.kind, case.params.primary_preprocessing) if case.auto_k is not None else None
        _WANT[case.name] = bs.run_batch_host(orc, api, *case.batch(), primary_g=hook, splits=case.splits)
    return _WANT[case.name]


def _check(prod, eng, orc, orc_ext, case, route="flags0"):
    """The case through one route against the oracle's call loop; returns the
    oracle's frames and the launch counters' increase."""
    want = _want(orc, orc_ext, case)
    with Launches(prod) as l:
        if route == "host":
            got = bs.run_batch_host(prod, api, *case.batch(), tails=True, splits=case.splits)
        else:
            flags = ROUTES[route] | (api.GPU_AUTO_RICE if case.auto_k is not None else 0)
            got = bs.run_batch_gpu(prod, eng, api, *case.batch(), flags=flags, tails=True, splits=case.splits)
    note = f"{case.name} [{route}]"
    bad = [(f, api.error_name(g[0]) if api.is_error(g[0]) else g[0], api.error_name(w[0]) if api.is_error(w[0]) else w[0])
           for f, (g, w) in enumerate(zip(got[0], want[0])) if g != w]
    assert not bad, f"{note}: frames (index, got, want) {bad[:6]}"
    for c, (g, w) in enumerate(zip(got[1], want[1])):
        assert g[:3] == w[:3], f"{note}: context {c} (identifier, sequence number, model size) {g[:3]} want {w[:3]}"
        assert g[3] == w[3], f"{note}: context {c}: work buffer differs at byte {first_diff(g[3], w[3])}"
    assert not got[2], f"{note}: (frame, offset) written at or behind the capacity {case.cap}: {got[2][:6]}"
    return want[0], l


def _fits(frames, nctx):
    """the oracle alone decides which frames fit: at least four of each"""
    ok = sum(not api.is_error(r) for r, _ in frames)
    small = sum(r == lc.TOO_SMALL for r, _ in frames)
    assert ok >= 4 and small >= 4 and ok + small == nctx, (ok, small)


# ---- a. capacity -------------------------------------------------------------

@pytest.mark.parametrize("res", range(8))
@pytest.mark.parametrize("k", (0, 5))
def test_capacity_rice_lb0(prod, eng, orc, orc_ext, k, res):
    """Rice kernel, vector look-back: nine frames of two segments (a frame
    count that is no multiple of 8), sizes S-4 .. S+4 at capacity S."""
    for ck in (0, 1):
        case = lc.capacity(orc, "rice_lb0", ("u16", "i16")[k & 1], k & 1, sc.ZERO, 1 << k, 0, 2 * SEG, 9, res, ck)
        frames, l = _check(prod, eng, orc, orc_ext, case)
        l.only(LB0, 1)
        _fits(frames, 9)


@pytest.mark.parametrize("res", range(8))
def test_capacity_rice_lb1(prod, eng, orc, orc_ext, res):
    """Rice kernel, scalar look-back: 8 frames x 17 segments, one context per
    frame (one launch through a frame list, as
    test_lookback_capacity_clipping_batch), sizes S-3 .. S+4 at capacity S."""
    k, pre = ((3, 1), (5, 0))[res & 1]
    for ck in (0, 1):
        case = lc.capacity(orc, "rice_lb1", ("u16", "i16")[res & 1], pre, sc.ZERO, 1 << k, 0, 17 * SEG, 8, res, ck)
        frames, l = _check(prod, eng, orc, orc_ext, case)
        l.only(LB1, 1)
        _fits(frames, 8)


@pytest.mark.parametrize("coder", sorted(lc.CODERS))
@pytest.mark.parametrize("kind", ("u16", "i16_in_i32"))
@pytest.mark.parametrize("n", (4160, 16385))
def test_capacity_encode(prod, eng, orc, orc_ext, n, kind, coder):
    """encode_kernel (a g that is no power of two, k = 8, MULTI; partial
    segments; 16385 samples: two or three segments, a look-back): nine frames
    S-4 .. S+4 at capacity S, every S mod 8, checksum off and on."""
    enc, g, outl = lc.CODERS[coder]
    for res in range(8):
        for ck in (0, 1):
            case = lc.capacity(orc, "encode", kind, (res + ck) & 1, enc, g, outl, n, 9, res, ck)
            frames, l = _check(prod, eng, orc, orc_ext, case)
            l.only(ENCODE, 1)
            _fits(frames, 9)


@pytest.mark.parametrize("n,kind", ((4160, "u16"), (16385, "i16_in_i32")))
def test_capacity_uncompressed(prod, eng, orc, orc_ext, n, kind):
    """UNCOMPRESSED frames have one size R, so the capacity moves instead:
    R-4 .. R+4, checksum off and on."""
    fit = 0
    for ck in (0, 1):
        for d in range(-4, 5):
            case = lc.capacity_raw(orc, kind, n, d, ck)
            frames, l = _check(prod, eng, orc, orc_ext, case)
            l.only(ENCODE, 1)
            assert all((not api.is_error(r)) == (d >= 0) for r, _ in frames), (ck, d)
            fit += d >= 0
    assert fit == 10


@pytest.mark.parametrize("which", ("i16_in_i32", "u16"))
def test_capacity_auto(prod, eng, orc, orc_ext, which):
    """encode_kernel's fused CMP_GPU_AUTO_RICE form (32-bit samples; partial
    16-bit frames): the frames select k = 3 (k = 5), the oracle codes them
    with the g its rule selects (the primary_g hook of run_batch_host)."""
    n, k = {"i16_in_i32": (16385, 3), "u16": (4160, 5)}[which]
    for res in range(8):
        for ck in (0, 1):
            case = lc.capacity(orc, "auto", which, res & 1, sc.ZERO, 1 << k, 0, n, 9, res, ck, k)
            frames, l = _check(prod, eng, orc, orc_ext, case)
            l.only(ENCODE, 1)
            _fits(frames, 9)
            assert all(api.parse_header(b)["encoder_param"] == 1 << k for _, b in frames if b is not None)


@pytest.mark.parametrize("which,stat", (("rice", RICE_STREAM), ("encode", ENCODE_STREAM)))
def test_capacity_stream(prod, eng, which, stat):
    """Payload-only streams of exactly `size` bytes at cap == size and
    cap == size + 1 (size - 1: test_gpu_stream.py), two residues of size mod
    8, through both stream kernels."""
    for res in (0, 5):
        x, kind, pre, enc, g, outl, size = lc.stream(None, which, res)
        want = streams.oracle_stream(x, kind, pre, enc, g, outl)
        assert want[0] == size and size % 8 == res
        for cap in (size, size + 1):
            assert streams.oracle_stream(x, kind, pre, enc, g, outl, cap=cap) == want
            with Launches(prod) as l:
                got = gpu_stream(eng, x, kind, pre, enc, g, outl, cap=cap)
            l.only(stat, 1)
            assert got == want, (which, res, cap, got[0], want[0])


# ---- b. fallback -------------------------------------------------------------

def _fallback_edges(case, frames):
    """raw-1 and raw stay compressed, raw+1 falls back, as the primary and as
    the secondary pass: the test cannot pass by missing the edge"""
    edges = lc.fallback_edges(case, frames)
    for sec in (0, 1):
        assert [edges[(d, sec)] for d in lc.FB_OFFS] == ["compressed"] * 3 + ["raw"] * 2, (case.name, sec, edges)


@pytest.mark.parametrize("worst", (False, True), ids=("cap_raw", "cap_worst"))
@pytest.mark.parametrize("ck", (0, 1))
@pytest.mark.parametrize("route", ("host", "host_stepped", "stepwise"))
def test_fallback_routes(prod, eng, orc, orc_ext, route, ck, worst):
    """Ten contexts of five 8192-sample frames whose edge frame compresses to
    raw-2 .. raw+2 bytes, through the host API (cmp_compress_* in a loop),
    CMP_GPU_HOST_STEPPED (batch_exact) and CMP_GPU_STEPWISE
    (batch_device_exact: a fallback step per acquisition)."""
    case = lc.fallback(orc, ("u16", "i16_in_i32")[ck], 8192, ck, worst)
    frames, l = _check(prod, eng, orc, orc_ext, case, route)
    _fallback_edges(case, frames)
    d = l.delta
    assert d[WALK_CTX] == 0 and d[WALK_SEG] == 0 and d[ENCODE] > 0, l.named()
    assert d[FB_STEP] == (lc.FB_FPC + 1 if route == "stepwise" else 0), l.named()


@pytest.mark.parametrize("worst", (False, True), ids=("cap_raw", "cap_worst"))
@pytest.mark.parametrize("ck", (0, 1))
def test_fallback_segment_walk(prod, eng, orc, orc_ext, ck, worst):
    """The same batch with flags 0: too few contexts for the context walk, so
    the segment walk codes every frame at the raw size as capacity and the
    contexts with a frame that did not fit run again on the device state
    machine (batch_walk_spec)."""
    case = lc.fallback(orc, ("u16", "i16_in_i32")[ck], 8192, ck, worst)
    frames, l = _check(prod, eng, orc, orc_ext, case)
    _fallback_edges(case, frames)
    d = l.delta
    assert d[WALK_SEG] == 1 and d[WALK_CTX] == 0, l.named()
    assert d[FB_STEP] == 4 * (lc.FB_FPC + 1), l.named()  # the four contexts whose edge is above raw, one by one


@pytest.mark.parametrize("worst", (False, True), ids=("cap_raw", "cap_worst"))
@pytest.mark.parametrize("ck", (0, 1))
def test_fallback_context_walk(prod, eng, orc, orc_ext, ck, worst):
    """130 contexts of 64 Ki-sample frames (the ten contexts thirteen times)
    with flags 0: the context walk resolves every fallback on the chip
    (batch_walk_fb), one launch."""
    case = lc.fallback(orc, ("i16_in_i32", "u16")[ck], 65536, ck, worst, 13)
    frames, l = _check(prod, eng, orc, orc_ext, case)
    _fallback_edges(case, frames)
    d = l.delta
    assert d[WALK_CTX] == 1 and d[WALK_SEG] == 0 and d[FB_STEP] == 0 and d[ENCODE] == 0, l.named()


# ---- c. model fail bit -------------------------------------------------------

@pytest.mark.parametrize("res", (0, 1, 7))
@pytest.mark.parametrize("route", sorted(ROUTES))
def test_model_fail_bit(prod, eng, orc, orc_ext, route, res):
    """MODEL passes without the fallback at a capacity below the frame (cap
    mod 8 = res): the sample that ends on bit 64 (cap / 8) + 63 keeps its new
    model, the sample that ends on the next bit is the first that keeps the
    old one, and so is an escape of which only the second piece crosses.  The
    work buffer is compared byte for byte, and the next frame, which is coded
    against it.  Without the fallback no walk takes such a batch (cmp_batch.c
    walk_prepare: exact mode needs the fallback): flags 0 is encode_kernel
    with a model under the device state machine, asserted."""
    case = lc.failbit(orc, ("u16", "i16_in_i32", "i16")[res % 3], 12288, res, res & 1)
    frames, l = _check(prod, eng, orc, orc_ext, case, route)
    assert [api.is_error(r) for r, _ in frames] == [False, True, False] * 3
    d = l.delta
    assert d[WALK_CTX] == 0 and d[WALK_SEG] == 0 and d[ENCODE] > 0, l.named()
    assert d[FB_STEP] == (4 if route in ("stepwise", "flags0") else 0), l.named()


# ---- d. the 24-bit size field ------------------------------------------------

@pytest.mark.parametrize("family,stat", (("rice", LB0), ("encode", ENCODE)))
def test_size_field_24bit(prod, eng, orc, orc_ext, family, stat):
    """Frames of 0xFFFFFE and 0xFFFFFF bytes are written, one of 0x1000000
    bytes is HDR_CMP_SIZE_TOO_LARGE: through the Rice kernel (511 whole
    segments) and through encode_kernel (8 388 000 samples).  The last frame
    fails, so the context stays at sequence number 0 (cmp.c:321-338): a batch
    whose coder can pass the field (g = 1: 17 bits a sample) runs step by
    step, one launch per frame.  (As first written, cmp_batch_compress ran it
    in one asynchronous launch and left the context at sequence number 1.)"""
    case = lc.size24(orc, family)
    frames, l = _check(prod, eng, orc, orc_ext, case)
    l.only(stat, 3)
    assert [r for r, _ in frames] == [0xFFFFFE, 0xFFFFFF, lc.TOO_LARGE]


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_size_field_24bit_call_by_call(prod, eng, orc, orc_ext, route):
    """One frame per cmp_gpu_compress call on a context with secondary passes:
    after the frame of 0x1000000 bytes the next call is a primary pass again,
    the one after it a secondary pass.  (As first written, a one-frame call
    was asynchronous whatever its coder and advanced the context past the
    failed frame, so the second call coded a secondary pass.)"""
    case = lc.size24_calls(orc)
    frames, l = _check(prod, eng, orc, orc_ext, case, route)
    assert frames[0][0] == lc.TOO_LARGE
    assert [api.parse_header(b)["sequence_number"] for _, b in frames[1:]] == [0, 1]
    assert l.delta[WALK_CTX] == 0 and l.delta[WALK_SEG] == 0, l.named()


@pytest.mark.parametrize("n", (8388599, 8388600))
@pytest.mark.parametrize("route", sorted(ROUTES))
def test_fallback_24bit(prod, eng, orc, orc_ext, route, n):
    """A fallback context with secondary passes whose noise frame falls back
    to a raw frame of 16 777 214 bytes (written) or 16 777 216 bytes
    (HDR_CMP_SIZE_TOO_LARGE: the context stays at its primary pass), then two
    frames whose pass depends on that outcome."""
    case = lc.fb24(orc, n)
    frames, l = _check(prod, eng, orc, orc_ext, case, route)
    if n == 8388599:
        assert frames[0][0] == 16777214 and api.parse_header(frames[0][1])["encoder_type"] == 0
    else:
        assert frames[0][0] == lc.TOO_LARGE
    assert not api.is_error(frames[2][0]) and api.parse_header(frames[2][1])["sequence_number"] == 1
    d = l.delta
    assert d[WALK_CTX] == 0 and d[WALK_SEG] == 0, l.named()
    assert d[FB_STEP] == (4 if route in ("stepwise", "flags0") else 0), l.named()
