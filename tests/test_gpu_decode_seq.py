"""Whole MODEL sequences on the GPU (cmp_gpu_decompress_sequences).  Truth is
the encoder: the frames come from the CPU oracle's call loop (one context per
sequence, one cmp_compress_* per acquisition), the expected output is the
source samples' low 16 bits, bit-exact, and the expected model is the oracle's
work buffer after its last call, bytewise."""
import numpy as np
import pytest

import configs
from conftest import load_pkg

pytestmark = pytest.mark.gpu
pkg = load_pkg()
api = pkg.cmpapi

TILE = 2048  # samples a chain workgroup covers (SEQ_TILE in decode.hip)
SIZES = (1, 7, 8, 9, 4097, TILE - 1, TILE, TILE + 1)
RATES = (0, 11, 16)
ITERS = (1, 2, 15)
NCTX, FPC = 3, 6


@pytest.fixture(scope="module")
def eng(prod):
    if not prod.gpu_available():
        pytest.fail("GPU test run without a usable HIP device")
    e = prod.engine()
    yield e
    e.close()


def make_x(kind, n, rng, base, spread=40):
    """One acquisition around `base` (int64 walk); values cover both halves of
    the 16-bit range, so the signed and unsigned model updates differ."""
    lo = ((base + rng.integers(-spread, spread + 1, n)) & 0xFFFF).astype(np.uint16)
    if kind == "u16":
        return lo
    if kind == "i16":
        return lo.view(np.int16)
    junk = rng.integers(0, 1 << 16, n).astype(np.uint32) << 16
    return (junk | lo).view(np.int32)


def low16(x):
    return (np.asarray(x).astype(np.int64) & 0xFFFF).astype(np.uint16)


def oracle_sequence(orc, params, kind, n, rng, fpc=FPC, noisy=()):
    """One context's frames from the oracle's call loop: (frames, inputs, the
    model it holds at the end)."""
    ctx = api.CmpContext()
    wbs = orc.cal_work_buf_size(params, (4 if kind == "i16_in_i32" else 2) * n)
    assert not api.is_error(wbs), api.error_name(wbs)
    wb = api.aligned_empty(max(wbs, 2), fill=0)
    assert not api.is_error(orc.initialise(ctx, params, wb if wbs else None, wbs))
    base = np.cumsum(rng.integers(-300, 301, n)) + int(rng.integers(0, 1 << 16))
    frames, xs = [], []
    cap = 26 + 6 * n + 64
    for a in range(fpc):
        x = make_x(kind, n, rng, base, 30000 if a in noisy else 40)
        dst = api.aligned_empty(cap)
        r = orc.compress(kind, ctx, dst, cap, x)
        assert not api.is_error(r), api.error_name(r)
        frames.append(bytes(dst[:r]))
        xs.append(low16(x))
    model = np.frombuffer(bytes(wb[:2 * n]), dtype=np.uint16).copy() if wbs else None
    return frames, xs, model


def run_seq(eng, kind, frames, nctx, fpc, nmax, dstride=None, mstride=None, want_model=True, want_ck=False,
            flags=0, model_in=None, model_n_in=None):
    """Upload frames (c-major) and decode them as nctx sequences of fpc.
    Returns (rc, statuses, rows, model rows, model_n, checksum_ok)."""
    import torch
    assert len(frames) == nctx * fpc
    cap = (max(24, max(len(f) for f in frames)) + 7) // 8 * 8
    nf = len(frames)
    host = np.zeros(nf * cap, dtype=np.uint8)
    for i, f in enumerate(frames):
        host[i * cap:i * cap + len(f)] = np.frombuffer(f, dtype=np.uint8)
    src = torch.from_numpy(host).cuda()
    dstride = dstride or 2 * nmax
    mstride = mstride or 2 * nmax
    dst = torch.zeros(nf * dstride + 16, dtype=torch.uint8, device="cuda")
    st = torch.zeros(nf, dtype=torch.int32, device="cuda")
    mod = torch.zeros(nctx * mstride + 16, dtype=torch.uint8, device="cuda")
    mn = torch.zeros(nctx, dtype=torch.int32, device="cuda")
    if model_in is not None:
        mod[:nctx * mstride] = torch.from_numpy(model_in.reshape(-1).view(np.uint8).copy()).cuda()
        mn[:] = torch.from_numpy(np.asarray(model_n_in, dtype=np.int32)).cuda()
    ck = torch.full((nf,), 77, dtype=torch.uint8, device="cuda")
    rc = eng.decompress_sequences(kind, src.data_ptr(), cap, cap, nctx, fpc, dst.data_ptr(), dstride, nmax,
                                  st.data_ptr(), mod.data_ptr() if want_model else 0, mstride,
                                  mn.data_ptr() if want_model else 0, ck.data_ptr() if want_ck else 0, flags)
    assert eng.synchronize() == 0
    status = [int(s) & 0xFFFFFFFF for s in st.cpu().numpy()]
    out = dst.cpu().numpy()
    rows = [out[i * dstride:i * dstride + 2 * nmax].view(np.uint16) for i in range(nf)]
    m = mod.cpu().numpy()
    mrows = [m[c * mstride:c * mstride + 2 * nmax].view(np.uint16) for c in range(nctx)]
    return rc, status, rows, mrows, [int(v) for v in mn.cpu().numpy()], [int(v) for v in ck.cpu().numpy()]


def name(s):
    return api.error_name(s) if api.is_error(s) else s


def check_ok(status, rows, xs, which=None):
    for i, x in enumerate(xs):
        if which is not None and i not in which:
            continue
        assert status[i] == len(x), (i, name(status[i]))
        assert np.array_equal(rows[i][:len(x)], x), i


def params(primary=1, sec_enc=2, rate=11, iters=15, **kw):
    d = dict(primary_preprocessing=primary, primary_encoder_type=1, primary_encoder_param=16,
             secondary_iterations=iters, secondary_preprocessing=3, secondary_encoder_type=sec_enc,
             secondary_encoder_param=8, secondary_encoder_outlier=107, model_rate=rate)
    d.update(kw)
    return api.CmpParams(**d)


def build(orc, prm, kind, ns, rng, fpc=FPC, noisy=()):
    """len(ns) contexts (context c has ns[c] samples per frame); prm: one
    CmpParams or one per context."""
    frames, xs, models = [], [], []
    for c, n in enumerate(ns):
        p = prm[c] if isinstance(prm, (list, tuple)) else prm
        f, x, m = oracle_sequence(orc, p, kind, n, rng, fpc, noisy)
        frames += f
        xs += x
        models.append(m)
    return frames, xs, models


@pytest.mark.parametrize("kind", ["u16", "i16", "i16_in_i32"])
def test_roundtrip(eng, orc, kind):
    """3 contexts x 6 frames per call: every primary preprocessing x secondary
    encoder x size, the model rates and secondary_iterations cycling so that
    each (size, rate, iterations) triple occurs; samples of every frame and the
    final models against the oracle."""
    rng = np.random.default_rng({"u16": 21, "i16": 22, "i16_in_i32": 23}[kind])
    idx = 0
    for primary in (0, 1, 2):
        for sec_enc in (0, 1, 2):
            for n in SIZES:
                rate, iters = RATES[idx % 3], ITERS[(idx // 3) % 3]
                idx += 1
                prm = params(primary, sec_enc, rate, iters)
                frames, xs, models = build(orc, prm, kind, [n] * NCTX, rng)
                pres = [f[15] >> 4 for f in frames[:FPC]]
                assert pres[0] == primary and 3 in pres
                rc, status, rows, mrows, mn, _ = run_seq(eng, kind, frames, NCTX, FPC, n)
                tag = (primary, sec_enc, n, rate, iters)
                assert rc == 0, (tag, name(rc))
                for i, x in enumerate(xs):
                    assert status[i] == n, (tag, i, name(status[i]))
                    assert np.array_equal(rows[i][:n], x), (tag, i)
                assert mn == [n] * NCTX, tag
                for c in range(NCTX):
                    assert mrows[c][:n].tobytes() == models[c].tobytes(), (tag, c)


def test_signed_and_unsigned_updates_differ(orc):
    """The inputs above do pin the extension: the same 16-bit patterns give
    different models under the u16 and the i16 rule (CPU only)."""
    rng = np.random.default_rng(5)
    st = rng.bit_generator.state
    _, _, mu = oracle_sequence(orc, params(rate=11), "u16", 4097, rng)
    rng.bit_generator.state = st
    _, _, mi = oracle_sequence(orc, params(rate=11), "i16", 4097, rng)
    assert not np.array_equal(mu, mi)


def test_fallback_in_mid_sequence(eng, orc):
    """Raw fallback frames (sequence number 0, NONE + UNCOMPRESSED) between
    MODEL frames: the model restarts from their samples."""
    rng = np.random.default_rng(31)
    n = 4097
    prm = params(1, 2, 11, 15, uncompressed_fallback_enabled=1)
    frames, xs, models = build(orc, prm, "u16", [n] * NCTX, rng, noisy=(2, 3))
    raw_mid = [i for i, f in enumerate(frames) if i % FPC and f[15] == 0 and f[14] == 0]
    assert raw_mid, "no raw fallback frame in mid-sequence"
    assert any((frames[i + 1][15] >> 4) == 3 for i in raw_mid if (i + 1) % FPC), "no MODEL frame after a fallback"
    rc, status, rows, mrows, mn, _ = run_seq(eng, "u16", frames, NCTX, FPC, n)
    assert rc == 0
    check_ok(status, rows, xs)
    assert mn == [n] * NCTX
    for c in range(NCTX):
        assert mrows[c][:n].tobytes() == models[c].tobytes(), c


@pytest.mark.parametrize("kind", ["u16", "i16"])
def test_continuation(eng, orc, kind):
    """Frames 0-2 in one call and 3-5 in a second one with MODEL_IN equal one
    call; without the flag the second call's leading MODEL frames have no model."""
    rng = np.random.default_rng(41)
    n = TILE + 9
    frames, xs, models = build(orc, params(2, 1, 11, 15), kind, [n] * NCTX, rng)
    rc, status, rows, mrows, mn, _ = run_seq(eng, kind, frames, NCTX, FPC, n)
    assert rc == 0
    check_ok(status, rows, xs)
    first = [frames[c * FPC + a] for c in range(NCTX) for a in range(3)]
    second = [frames[c * FPC + a] for c in range(NCTX) for a in range(3, 6)]
    rc, s1, r1, m1, n1, _ = run_seq(eng, kind, first, NCTX, 3, n)
    assert rc == 0 and s1 == [n] * 9 and n1 == [n] * NCTX
    rc, s2, r2, m2, n2, _ = run_seq(eng, kind, second, NCTX, 3, n, flags=pkg.SEQ_MODEL_IN,
                                    model_in=np.stack(m1), model_n_in=n1)
    assert rc == 0 and s2 == [n] * 9 and n2 == [n] * NCTX
    for c in range(NCTX):
        for a in range(3):
            assert np.array_equal(r1[c * 3 + a], rows[c * FPC + a]), (c, a)
            assert np.array_equal(r2[c * 3 + a], rows[c * FPC + 3 + a]), (c, a)
        assert np.array_equal(m2[c], mrows[c]) and m2[c][:n].tobytes() == models[c].tobytes(), c
    rc, s3, _, _, n3, _ = run_seq(eng, kind, second, NCTX, 3, n, model_in=np.stack(m1), model_n_in=n1)
    assert rc == 0
    assert [name(s) for s in s3] == ["PARAMS_INVALID"] * 9 and n3 == [0] * NCTX


def test_broken_chains(eng, orc):
    rng = np.random.default_rng(51)
    n = 4097
    # secondary_iterations 3: P M M M P M
    frames, xs, models = build(orc, params(1, 2, 11, 3), "u16", [n] * NCTX, rng)
    assert [f[15] >> 4 for f in frames[:FPC]] == [1, 3, 3, 3, 1, 3]
    bad = list(frames)
    b = bytearray(bad[1 * FPC + 2])
    b[1] ^= 0x55  # version id
    bad[1 * FPC + 2] = bytes(b)
    rc, status, rows, mrows, mn, _ = run_seq(eng, "u16", bad, NCTX, FPC, n)
    assert rc == 0
    assert name(status[FPC + 2]) == "INT_HDR" and name(status[FPC + 3]) == "PARAMS_INVALID"
    check_ok(status, rows, xs, set(range(3 * FPC)) - {FPC + 2, FPC + 3})
    assert mn == [n] * NCTX
    for c in range(NCTX):
        assert mrows[c][:n].tobytes() == models[c].tobytes(), c

    # a MODEL frame of another original size; the MODEL frames after it have no model
    bad = list(frames)
    b = bytearray(bad[1])
    b[5:8] = (2 * (n - 1)).to_bytes(3, "big")
    bad[1] = bytes(b)
    rc, status, rows, _, mn, _ = run_seq(eng, "u16", bad, NCTX, FPC, n)
    assert rc == 0
    assert [name(s) for s in status[:4]] == [n, "SRC_SIZE_MISMATCH", "PARAMS_INVALID", "PARAMS_INVALID"]
    check_ok(status, rows, xs, {0} | set(range(4, 3 * FPC)))

    # no such model rate; the context ends without a model
    bad = list(frames)
    b = bytearray(bad[2 * FPC + 5])
    assert b[16] == 11
    b[16] = 17
    bad[2 * FPC + 5] = bytes(b)
    rc, status, rows, _, mn, _ = run_seq(eng, "u16", bad, NCTX, FPC, n)
    assert rc == 0
    assert name(status[2 * FPC + 5]) == "INT_HDR"
    check_ok(status, rows, xs, set(range(3 * FPC - 1)))
    assert mn == [n, n, 0]


@pytest.mark.parametrize("kind", ["u16", "i16_in_i32"])
def test_unaligned_rows(eng, orc, kind):
    """dst_stride and model_stride that are no multiple of 16, odd n: the
    2-byte path of the chain."""
    rng = np.random.default_rng(61)
    n = TILE + 77
    frames, xs, models = build(orc, params(1, 1, 11, 2), kind, [n] * NCTX, rng)
    rc, status, rows, mrows, mn, _ = run_seq(eng, kind, frames, NCTX, FPC, n, dstride=2 * n + 2, mstride=2 * n + 6)
    assert rc == 0
    check_ok(status, rows, xs)
    for c in range(NCTX):
        assert mrows[c][:n].tobytes() == models[c].tobytes(), c


def test_checksums(eng, orc):
    rng = np.random.default_rng(71)
    ns = [100, 4097, 9, 333]
    prm = [params(1, 2, 11, 15, checksum_enabled=1), params(2, 1, 16, 2, checksum_enabled=1),
           params(0, 0, 0, 15, checksum_enabled=1), params(1, 2, 11, 15)]
    frames, xs, models = build(orc, prm, "u16", ns, rng)
    nmax, nctx = max(ns), len(ns)
    want = [1] * (3 * FPC) + [0] * FPC
    rc, status, rows, mrows, mn, ck = run_seq(eng, "u16", frames, nctx, FPC, nmax, want_ck=True)
    assert rc == 0
    check_ok(status, rows, xs)
    assert ck == want
    assert mn == ns
    # without checksum_ok nothing differs
    rc, status2, rows2, mrows2, mn2, ck2 = run_seq(eng, "u16", frames, nctx, FPC, nmax)
    assert rc == 0 and status2 == status and mn2 == mn and ck2 == [77] * len(frames)
    assert all(np.array_equal(a, b) for a, b in zip(rows, rows2))
    assert all(np.array_equal(a, b) for a, b in zip(mrows, mrows2))
    # one trailer bit; one sample bit of an UNCOMPRESSED (MODEL) frame, the last of its context
    bad = list(frames)
    b = bytearray(bad[FPC + 3])
    b[-2] ^= 0x10
    bad[FPC + 3] = bytes(b)
    f = 2 * FPC + 5
    assert frames[f][15] & 7 == 0 and frames[f][15] >> 4 == 3
    b = bytearray(bad[f])
    b[22 + 2 * 4] ^= 0x01
    bad[f] = bytes(b)
    rc, status3, rows3, _, _, ck3 = run_seq(eng, "u16", bad, nctx, FPC, nmax, want_ck=True)
    assert rc == 0 and status3 == status
    want3 = list(want)
    want3[FPC + 3] = want3[f] = 2
    assert ck3 == want3
    assert rows3[f][4] == (int(xs[f][4]) + 0x100) & 0xFFFF or rows3[f][4] == (int(xs[f][4]) - 0x100) & 0xFFFF


def test_full_size(prod, eng):
    """cfg5_model's frames from the GPU encoder (32 of its 256 streams, to keep
    the test to seconds): decode equals the synthesized inputs' low halves."""
    import torch
    cfg = dict(configs.CONFIGS["cfg5_model"])
    cfg["nctx"] = 32
    frames, _, _ = configs.gpu_frames(prod, eng, cfg)
    n, nctx, fpc = cfg["n"], cfg["nctx"], cfg["fpc"]
    assert sum((f[15] >> 4) == 3 for f in frames) == nctx * (fpc - 1)
    rc, status, rows, _, mn, _ = run_seq(eng, cfg["kind"], frames, nctx, fpc, n)
    assert rc == 0 and status == [n] * len(frames) and mn == [n] * nctx
    src = torch.empty(len(frames) * 4 * n, dtype=torch.uint8, device="cuda")
    assert eng.synthesize(src.data_ptr(), 4, cfg["seed"], 0, n, len(frames), 4 * n, cfg["W"]) == 0
    assert eng.synchronize() == 0
    x = (src.cpu().numpy().view(np.uint32).reshape(len(frames), n) & 0xFFFF).astype(np.uint16)
    for i in range(len(frames)):
        assert np.array_equal(rows[i], x[i]), i
