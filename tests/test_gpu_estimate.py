"""cmp_gpu_estimate on the GPU against the CPU oracle: the exact payload bits of
every frame under every candidate (NONE, DIFF, IWT and MODEL preprocessing;
UNCOMPRESSED, GOLOMB_ZERO and GOLOMB_MULTI; Rice and general g), the choice
in best, the frame sizes that follow from the bits, and what the call may
write.  Exact bits: estimate_helpers.exact_bits."""
import functools
import os
import zlib

import numpy as np
import pytest

import estimate_helpers as eh
import streams
from conftest import load_pkg
from estimate_helpers import DIFF, IWT, MODEL, MULTI, NONE, RAW, ZERO
from rice_helpers import Launches

pytestmark = pytest.mark.gpu
api = load_pkg().cmpapi
P = api.CmpParams

# csrc/estimate.hip: EST_CHUNK samples per workgroup and step, EST_SLICE per
# workgroup, EST_GROUP candidates per sizing launch
CHUNK = 4096
SLICE = 16 * CHUNK
GROUP = 16
KINDS = ("u16", "i16", "i16_in_i32")

SHAPES = [1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1, SLICE - 1, SLICE, SLICE + 1,
          2 * SLICE + 17, 200001]
# NONE and DIFF; ZERO, MULTI and UNCOMPRESSED; g in {1, 2, 3, 32, 1055, 32768, 65535}; outliers {1, 107, 399}
MIX = [(NONE, ZERO, 1, 0), (DIFF, ZERO, 2, 0), (NONE, ZERO, 32, 0), (DIFF, ZERO, 32, 0), (DIFF, ZERO, 32768, 0),
       (NONE, ZERO, 3, 0), (DIFF, ZERO, 1055, 0), (NONE, ZERO, 65535, 0), (NONE, MULTI, 1, 1),
       (DIFF, MULTI, 2, 107), (DIFF, MULTI, 3, 399), (NONE, MULTI, 32, 107), (DIFF, MULTI, 1055, 399),
       (NONE, MULTI, 32768, 1), (DIFF, MULTI, 65535, 107), (NONE, RAW, 0, 0)]
RICE16 = [(NONE, ZERO, 1 << k, 0) for k in range(16)]


@pytest.fixture(scope="module")
def eng(prod):
    if not prod.gpu_available():
        pytest.fail("GPU test run without a usable HIP device")
    e = prod.engine()
    yield e
    e.close()


def rng_of(*what):
    return np.random.default_rng(zlib.crc32("/".join(str(w) for w in ("estimate",) + what).encode()))


@functools.lru_cache(maxsize=None)
def shape_case(n):
    """Three frames of n patterns and their exact bits under MIX: computed
    once, shared by the sample types (only the low halves count) and left
    unchanged."""
    rng = rng_of("shape", n)
    los = [eh.low16(rng, n) for _ in range(3)]
    want = np.array([[eh.exact_bits(eh.residuals(lo, c[0]), *c[1:]) for c in MIX] for lo in los], dtype=np.uint64)
    for lo in los:
        lo.setflags(write=False)
    want.setflags(write=False)
    return los, want


@pytest.mark.parametrize("n", SHAPES)
def test_bits_vs_oracle_shapes(eng, orc_ext, n):
    los, want = shape_case(n)
    rng = rng_of("kinds", n)
    for kind in KINDS:
        frames = [eh.as_kind(rng, lo, kind) for lo in los]
        sb = frames[0].itemsize
        # 16-byte aligned frames, and frames one sample past a boundary (the guarded loads)
        for offset in (0, sb):
            bits, _ = eh.run(eng, kind, frames, MIX, offset=offset)
            assert (bits == want).all(), (kind, offset, np.argwhere(bits != want)[:5].tolist())
        for f, x in enumerate(frames):
            kbits = np.zeros(16, dtype=np.uint64)
            for pre in (NONE, DIFF):
                orc_ext.orc_select_rice_k(x.ctypes.data, n, 1 if sb == 4 else 0, pre, kbits.ctypes.data)
                for c, (cp, enc, g, outl) in enumerate(MIX):
                    if cp == pre and enc == ZERO and g & (g - 1) == 0:
                        assert int(want[f, c]) == int(kbits[g.bit_length() - 1]), (kind, f, c)
            for c, (pre, enc, g, outl) in enumerate(MIX):
                size, _ = streams.oracle_stream(x, kind, pre, enc, g, outl)
                assert (int(want[f, c]) + 7) // 8 == size, (kind, f, c)


@pytest.mark.parametrize("count", [1, GROUP + 1, 64])
def test_candidate_counts_and_duplicates(eng, count):
    # one candidate, one more than a group, the most a call takes; repeats included
    n = CHUNK + 17
    rng = rng_of("count", count)
    los = [eh.low16(rng, n) for _ in range(2)]
    cands = [MIX[int(i)] for i in rng.integers(0, len(MIX), count)]
    if count > 1:
        cands[-1] = cands[0]
    bits, _ = eh.run(eng, "u16", los, cands)
    ref = {}
    for f, lo in enumerate(los):
        for c, cand in enumerate(cands):
            if (f, cand) not in ref:
                ref[f, cand] = eh.exact_bits(eh.residuals(lo, cand[0]), *cand[1:])
            assert int(bits[f, c]) == ref[f, cand], (f, c, cand)
    if count > 1:
        assert (bits[:, -1] == bits[:, 0]).all()


@pytest.mark.parametrize("pre", [NONE, DIFF])
def test_best_is_the_auto_rice_rule(eng, orc_ext, pre):
    rng = rng_of("best", pre)
    n = 3001
    los = [eh.low16(rng, n) for _ in range(40)]
    cands = [(pre, ZERO, 1 << k, 0) for k in range(16)]
    bits, best = eh.run(eng, "i16", [lo.view(np.int16) for lo in los], cands)
    kbits = np.zeros(16, dtype=np.uint64)
    for f, lo in enumerate(los):
        k = orc_ext.orc_select_rice_k(lo.ctypes.data, n, 0, pre, kbits.ctypes.data)
        assert (bits[f] == kbits).all(), f
        assert int(best[f]) == k, (f, int(best[f]), k)
    assert len(set(best.tolist())) > 3  # the frames do not all choose alike


def test_best_tie_goes_to_the_lower_index(eng):
    # zeros cost 2 bits under ZERO g = 1 (k + 2) and under g = 2 (k + 1): a tie in bits and header
    x = np.zeros(777, dtype=np.uint16)
    for cands in ([(NONE, ZERO, 4, 0), (NONE, ZERO, 1, 0), (NONE, ZERO, 2, 0)],
                  [(NONE, ZERO, 4, 0), (NONE, ZERO, 2, 0), (NONE, ZERO, 1, 0), (DIFF, ZERO, 1, 0)]):
        bits, best = eh.run(eng, "u16", [x, x], cands)
        assert bits[0].tolist()[:3] in ([3 * 777, 2 * 777, 2 * 777],) and best.tolist() == [1, 1]


def test_best_takes_the_header_into_account(eng):
    # white noise: NONE + UNCOMPRESSED (a 16-byte header) wins exactly when 8 * 16 + 16 n is smaller
    rng = rng_of("white")
    n = 500
    los = [rng.integers(0, 1 << int(w), n).astype(np.uint16) for w in (16, 16, 15, 14, 12, 16, 15, 8)]
    cands = [(NONE, ZERO, 1 << 14, 0), (NONE, ZERO, 1 << 13, 0), (NONE, RAW, 0, 0), (NONE, ZERO, 1 << 11, 0),
             (DIFF, RAW, 0, 0)]
    bits, best = eh.run(eng, "u16", los, cands)
    raw_wins = 0
    for f in range(len(los)):
        assert int(bits[f, 2]) == 16 * n and int(bits[f, 4]) == 16 * n
        for c in (0, 1, 3):
            assert int(bits[f, c]) == eh.exact_bits(eh.residuals(los[f], NONE), *cands[c][1:]), (f, c)
        total = [8 * eh.header_bytes(c) + int(bits[f, i]) for i, c in enumerate(cands)]
        assert total[2] == 8 * 16 + 16 * n and total[4] == 8 * 22 + 16 * n
        # ties go to the lower index: 0 and 1 beat it at equal totals, 3 and 4 do not
        wins = all(total[2] < total[c] for c in (0, 1)) and all(total[2] <= total[c] for c in (3, 4))
        assert (int(best[f]) == 2) == wins, (f, total)
        assert int(best[f]) == total.index(min(total)), (f, total)
        raw_wins += int(best[f]) == 2
    assert 0 < raw_wins < len(los)


@pytest.mark.parametrize("kind", KINDS)
def test_model_bits_vs_oracle(eng, kind):
    rng = rng_of("model", kind)
    cands = [(MODEL, ZERO, 16, 0), (MODEL, MULTI, 3, 107), (MODEL, RAW, 0, 0), (MODEL, ZERO, 1055, 0)]
    for n, moff in ((1, 0), (17, 2), (CHUNK + 1, 0), (SLICE + 300, 0), (SLICE + 300, 2)):
        los = [eh.low16(rng, n) for _ in range(3)]
        models = [(lo.astype(np.int64) + np.round(rng.laplace(0, 9, n)).astype(np.int64) & 0xFFFF).astype(np.uint16)
                  for lo in los]
        bits, _ = eh.run(eng, kind, [eh.as_kind(rng, lo, kind) for lo in los], cands, models=models,
                         model_offset=moff)
        for f in range(3):
            res = eh.residuals(los[f], MODEL, models[f])
            for c, (_, enc, g, outl) in enumerate(cands):
                size, _ = streams.oracle_stream(res.view(np.uint16), "u16", NONE, enc, g, outl)
                assert (int(bits[f, c]) + 7) // 8 == size, (n, f, c)
                assert int(bits[f, c]) == eh.exact_bits(res, enc, g, outl), (n, f, c)


@pytest.mark.parametrize("checksum", [0, 1])
def test_model_against_a_real_sequence(prod, eng, orc, checksum):
    # the oracle's second frame of a context (primary NONE + UNCOMPRESSED, secondary MODEL): its model
    # is the first frame's samples
    rng = rng_of("sequence", checksum)
    n = 5003
    x0 = eh.low16(rng, n, walk=True)
    x1 = (x0.astype(np.int64) + np.round(rng.laplace(0, 5, n)).astype(np.int64) & 0xFFFF).astype(np.uint16)
    cand = (MODEL, ZERO, 8, 0)
    prm = P(primary_preprocessing=NONE, primary_encoder_type=RAW, secondary_iterations=3,
            secondary_preprocessing=MODEL, secondary_encoder_type=ZERO, secondary_encoder_param=8, model_rate=11,
            checksum_enabled=checksum)
    wbs = orc.cal_work_buf_size(prm, 2 * n)
    ctx, wb = api.CmpContext(), api.aligned_empty(wbs)
    assert not api.is_error(orc.initialise(ctx, prm, wb, wbs))
    cap = 6 * n + 64
    d = api.aligned_empty(cap)
    assert orc.compress("u16", ctx, d, cap, x0) == 16 + 2 * n + 4 * checksum
    want = orc.compress("u16", ctx, d, cap, x1)
    assert api.parse_header(d)["preprocessing"] == MODEL
    bits, _ = eh.run(eng, "u16", [x1], [cand], models=[x0])
    assert prod.estimate_frame_size(cand, int(bits[0, 0]), checksum) == want


def oracle_iwt_size(orc, kind, x, enc, g, outl, checksum):
    prm = P(primary_preprocessing=IWT, primary_encoder_type=enc, primary_encoder_param=g,
            primary_encoder_outlier=outl, checksum_enabled=checksum)
    wbs = (2 * x.size + 15) // 16 * 16
    ctx, wb = api.CmpContext(), api.aligned_empty(wbs)
    assert not api.is_error(orc.initialise(ctx, prm, wb, wbs))
    cap = 6 * x.size + 64
    r = orc.compress(kind, ctx, api.aligned_empty(cap), cap, x)
    assert not api.is_error(r), api.error_name(r)
    return r


IWT_CANDS = [(IWT, ZERO, 4, 0), (IWT, MULTI, 7, 107), (IWT, RAW, 0, 0)]


@pytest.mark.parametrize("n,kind", [(n, KINDS[i % 3]) for i, n in enumerate([1, 2, 3, 64, 127, 128, 4096, 16448, 65600])])
def test_iwt_frame_sizes_vs_oracle(prod, eng, orc, n, kind):
    rng = rng_of("iwt", n)
    los = [eh.low16(rng, n, walk=True) for _ in range(3)]
    frames = [eh.as_kind(rng, lo, kind) for lo in los]
    want = [[oracle_iwt_size(orc, kind, x, enc, g, outl, c & 1) for c, (_, enc, g, outl) in enumerate(IWT_CANDS)]
            for x in frames]
    got = {}
    # every chunk of frames the call cuts, and one frame per chunk (a test-only switch of estimate.hip)
    for forced in (None, "1"):
        for offset in (0, frames[0].itemsize):
            if forced:
                os.environ["AIRS_TEST_ESTIMATE_IWT_FRAMES"] = forced
            before = eh.estimate_stats(prod)
            try:
                bits, best = eh.run(eng, kind, frames, IWT_CANDS, offset=offset)
            finally:
                os.environ.pop("AIRS_TEST_ESTIMATE_IWT_FRAMES", None)
            # a chunk: two sizing launches (UNCOMPRESSED needs no coefficients and is sized from the
            # samples), one finishing launch, one transform
            chunks = 3 if forced else 1
            assert [a - b for a, b in zip(eh.estimate_stats(prod), before)] == [2 * chunks, chunks, chunks]
            got[forced, offset] = (bits.tolist(), best.tolist())
            for f in range(3):
                for c, cand in enumerate(IWT_CANDS):
                    assert prod.estimate_frame_size(cand, int(bits[f, c]), c & 1) == want[f][c], (forced, offset, f, c)
    assert all(v == got[None, 0] for v in got.values())


def test_model_beside_the_other_preprocessings(prod, eng, orc):
    rng = rng_of("beside")
    n = CHUNK + 130
    los = [eh.low16(rng, n, walk=True) for _ in range(3)]
    models = [np.roll(lo, 1) for lo in los]
    cands = [(MODEL, ZERO, 8, 0), (NONE, ZERO, 8, 0), (IWT, ZERO, 8, 0), (DIFF, MULTI, 5, 30), (IWT, MULTI, 2, 9),
             (MODEL, MULTI, 5, 30)]
    bits, best = eh.run(eng, "u16", los, cands, models=models)
    for f, lo in enumerate(los):
        total = []
        for c, cand in enumerate(cands):
            if cand[0] == IWT:
                assert prod.estimate_frame_size(cand, int(bits[f, c]), 0) == oracle_iwt_size(orc, "u16", lo, *cand[1:], 0)
            else:
                assert int(bits[f, c]) == eh.exact_bits(eh.residuals(lo, cand[0], models[f]), *cand[1:]), (f, c)
            total.append(8 * 22 + int(bits[f, c]))
        assert int(best[f]) == total.index(min(total))


def test_many_frames(eng, orc_ext):
    # more frames than a grid dimension past the first takes (65535)
    rng = rng_of("many")
    nf, n = 70000, 8
    x = np.round(rng.laplace(0, 6, (nf, n))).astype(np.int16)
    host = np.ascontiguousarray(x)
    import torch
    src = torch.from_numpy(host.view(np.uint8).reshape(-1)).cuda()
    bits = torch.zeros(nf * 2, dtype=torch.int64, device="cuda")
    best = torch.zeros(nf, dtype=torch.int32, device="cuda")
    cands = [(NONE, ZERO, 4, 0), (DIFF, ZERO, 1, 0)]
    assert eng.estimate("i16", src.data_ptr(), 2 * n, 2 * n, nf, cands, bits.data_ptr(), best.data_ptr()) == 0
    assert eng.synchronize() == 0
    got, gbest = bits.cpu().numpy().reshape(nf, 2), best.cpu().numpy()
    want = np.zeros((nf, 2), dtype=np.int64)
    kb = np.zeros(16, dtype=np.uint64)
    base, kbp = host.ctypes.data, kb.ctypes.data
    for f in range(nf):
        orc_ext.orc_select_rice_k(base + 2 * n * f, n, 0, NONE, kbp)
        want[f, 0] = kb[2]
        orc_ext.orc_select_rice_k(base + 2 * n * f, n, 0, DIFF, kbp)
        want[f, 1] = kb[0]
    assert (got == want).all(), np.argwhere(got != want)[:5].tolist()
    assert (gbest == (want[:, 1] < want[:, 0])).all()


def test_the_call_does_not_wait_for_the_device(eng):
    # behind tens of milliseconds of queued fills on the engine's stream (the null stream) the call
    # returns while the fills still run: it queued its launches and synchronised with nothing
    import torch
    rng = rng_of("async")
    n, nf = SLICE + 9, 4
    lo = eh.low16(rng, nf * n)
    src = torch.from_numpy(lo).cuda()
    bits = torch.zeros(nf * len(MIX), dtype=torch.int64, device="cuda")
    best = torch.zeros(nf, dtype=torch.int32, device="cuda")
    big = torch.empty(1 << 30, dtype=torch.uint8, device="cuda")

    def call():
        return eng.estimate("u16", src.data_ptr(), 2 * n, 2 * n, nf, MIX, bits.data_ptr(), best.data_ptr())

    assert call() == 0 and eng.synchronize() == 0  # the engine's scratch has its size now
    bits.zero_()
    done = torch.cuda.Event()
    for _ in range(40):
        big.fill_(7)
    done.record()
    assert call() == 0
    busy = not done.query()
    assert eng.synchronize() == 0
    assert busy, "the fills queued before the call had finished when it returned"
    got = bits.cpu().numpy().reshape(nf, len(MIX))
    for f in (0, nf - 1):
        for c in (3, 12):
            assert int(got[f, c]) == eh.exact_bits(eh.residuals(lo[f * n:(f + 1) * n], MIX[c][0]), *MIX[c][1:])


def test_launches_are_queued_and_best_is_optional(prod, eng):
    rng = rng_of("queued")
    n = 2 * SLICE + 5
    los = [eh.low16(rng, n) for _ in range(2)]
    cands = (MIX + RICE16)[:GROUP + 1]
    before = eh.estimate_stats(prod)
    with Launches(prod) as launches:
        with_best, best = eh.run(eng, "u16", los, cands)
    # one sizing launch per group of candidates and one finishing launch, queued by the call; no
    # transform without an IWT candidate, and none of the encoder's or the decoder's kernels
    assert [a - b for a, b in zip(eh.estimate_stats(prod), before)] == [2, 1, 0]
    assert not launches.named()
    without, none = eh.run(eng, "u16", los, cands, want_best=False)
    assert none is None and (with_best == without).all()
    for f, lo in enumerate(los):
        assert int(with_best[f, GROUP]) == eh.exact_bits(eh.residuals(lo, NONE), ZERO, 1, 0)
