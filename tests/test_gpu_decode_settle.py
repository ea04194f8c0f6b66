"""The GPU decoder on valid frames whose guessed parse starts are wrong
(csrc/decode.hip: warm_start, the settle loop of parse_wg and the rounds of
decode_frames).  Noise-like data, which the rest of the suite decodes, makes
every guess right; constant frames, ramps and 48-bit codewords do not.

Frames come from the oracle's encoder (settle_cases.py), never the GPU's.  A
host model of the parser (decode_model.py), anchored against the oracle, says
for each frame which guesses are wrong, what a parse begun there does, and how
many settle rounds (launches of dec_parse_kernel with first == 0, counted by
the device layer as AIRS_STAT_DECODE_ROUND) the decoder must take.  Every case
asserts the call's result, the status, the samples, the untouched guard behind
them and that count, after asserting that the model's result has the property
the case stands for."""
import random

import numpy as np
import pytest

import decode_model as dm
import settle_cases as sc
import streams
from conftest import load_pkg
from rice_helpers import DECODE_ROUND, Launches

pytestmark = pytest.mark.gpu
api = load_pkg().cmpapi

GUARD = 64      # samples behind the last row
FILL = 0xA5A5   # what dst holds before a call


@pytest.fixture(scope="module")
def eng(prod):
    if not prod.gpu_available():
        pytest.fail("GPU test run without a usable HIP device")
    e = prod.engine()
    yield e
    e.close()


@pytest.fixture(scope="module")
def cases(orc, orc_ext):
    """every case with its model result, made once"""
    out = {name: sc.case(orc, orc_ext, name) for name in sc.CASES}
    for c in out.values():
        sc.check_property(c, c.settled())
    return out


def status_text(s):
    return api.error_name(s) if api.is_error(s) else s


def decode_call(prod, eng, cs, n_max, vector):
    """One cmp_gpu_decompress call over the cases' frames.  vector: dst and its
    row stride are multiples of 16 (16-byte stores); else the stride is 2 *
    n_max with n_max odd (2-byte stores).  Asserts the call's result, every
    status and row and everything of dst the call must leave alone; returns the
    launch counters' increase."""
    import torch
    assert n_max >= max(c.n for c in cs)
    if vector:
        dstride = (2 * n_max + 15) // 16 * 16
    else:
        assert n_max % 2 == 1
        dstride = 2 * n_max
    row = dstride // 2
    cap = (max(len(c.frame) for c in cs) + 7) // 8 * 8
    host = np.zeros(len(cs) * cap, dtype=np.uint8)
    for i, c in enumerate(cs):
        host[i * cap:i * cap + len(c.frame)] = np.frombuffer(c.frame, dtype=np.uint8)
    src = torch.from_numpy(host).cuda()
    dst = torch.full((len(cs) * row + GUARD,), FILL - 0x10000, dtype=torch.int16, device="cuda")
    assert dst.data_ptr() % 16 == 0
    st = torch.zeros(len(cs), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    with Launches(prod) as l:
        r = eng.decompress(src.data_ptr(), cap, cap, len(cs), dst.data_ptr(), dstride, n_max, st.data_ptr())
        assert eng.synchronize() == 0
    assert r == 0, api.error_name(r)
    status = st.cpu().numpy().astype(np.uint32)
    out = dst.cpu().numpy().view(np.uint16)
    for i, c in enumerate(cs):
        assert int(status[i]) == c.n, (c.name, status_text(int(status[i])))
        got = out[i * row:(i + 1) * row]
        bad = np.flatnonzero(got[:c.n] != c.want)
        assert bad.size == 0, (c.name, f"{bad.size} samples differ, the first at {bad[0]}")
        assert (got[c.n:] == FILL).all(), (c.name, "samples behind row n overwritten")
    assert (out[len(cs) * row:] == FILL).all(), "guard behind the last row overwritten"
    assert all(v == 0 for i, v in enumerate(l.delta) if i != DECODE_ROUND), l.named()
    return l.delta[DECODE_ROUND]


def decode_both_ways(prod, eng, c, rounds):
    """the case alone in a call, through the 16-byte and the 2-byte store path"""
    for n_max, vector in ((c.n, True), (c.n | 1, False)):
        got = decode_call(prod, eng, [c], n_max, vector)
        assert got == rounds, (c.name, vector, got, rounds)


# ---------------------------------------------------------------- locked phase
@pytest.mark.parametrize("name", sc.LOCKED)
def test_locked_phase(prod, eng, cases, name):
    """Wrong guesses that stay wrong to the end of the frame and (L5 apart)
    meet no invalid codeword: each round hands the right start one workgroup
    on, so the decoder takes as many rounds as the frame has workgroups.
    L1 Rice k = 0 (17-bit escapes), one workgroup: only the chain inside it;
    L1a a payload of exactly one span, L1b one 16-bit subsequence more;
    L2 Rice k = 5; L3 the same codewords behind DIFF, whose inverse crosses the
    int16 wrap and several scan tiles; L4 the general parser; L5 wrong ranges
    that partly end in an invalid codeword."""
    c = cases[name]
    r = c.settled()
    if name == "L1a":
        assert c.n == 7710 and len(c.payload) == dm.SPAN_BYTES and c.stream.nsub == dm.DEC_WG
    if name == "L1b":
        assert c.n == 7711 and len(c.payload) == dm.SPAN_BYTES + 2 and c.stream.nsub == dm.DEC_WG + 1
        assert c.stream.nbits - dm.SPAN_BITS == 16 and c.bounds[-2] < dm.SPAN_BITS  # the rest of the last codeword
    if name == "L3":
        x = c.want.view(np.int16).astype(np.int64)
        assert (np.diff(x) < 0).sum() >= 2 and c.n > 3 * 4096  # int16 wraps, more than three DIFF tiles
    assert r.rounds == c.W == sc.CASES[name][5]
    decode_both_ways(prod, eng, c, r.rounds)


# ---------------------------------------------------------------- invalid-codeword wave
def test_invalid_codeword_wave_on_valid_data(prod, eng, cases):
    """B1: 48-bit codewords whose raw bits run into the next codeword's ones.
    Every wrongly begun range meets an invalid codeword, a workgroup's last
    exit is DEC_BAD and the next workgroup is handed it as its start."""
    c = cases["B1"]
    r = c.settled()
    assert set(np.diff(c.bounds)) == {48} and len(c.payload) == 6 * c.n
    assert r.handed_bad and all(f == "invalid" for f in r.fate.values()) and r.rounds == 3
    decode_both_ways(prod, eng, c, r.rounds)


# ---------------------------------------------------------------- partial redo
def test_partial_redo_recounts_the_workgroup(prod, eng, cases):
    """P1: workgroup 2 begins inside a constant run, so its first guess is
    wrong, but its parse falls into step in the noise behind the run and its
    last exit is right at once.  The one round redoes its first threads only,
    reports no change, and must still leave the workgroup's new count."""
    c = cases["P1"]
    r = c.settled()
    assert r.rounds == 1 and r.redone == [[2]] and r.first_wg_cnt[2] != r.wg_cnt[2]
    decode_both_ways(prod, eng, c, 1)


# ---------------------------------------------------------------- control
def test_control_has_nothing_to_settle(prod, eng, cases):
    c = cases["CTRL"]
    r = c.settled()
    assert c.W == 4 and not r.wrong and r.rounds == 1
    decode_both_ways(prod, eng, c, 1)


# ---------------------------------------------------------------- one call over mixed frames
MIXED = ("CTRL", "L1w5", "B1", "L4w2", "P1", "ONE")


@pytest.mark.parametrize("vector", [True, False], ids=["vec16", "scalar2"])
@pytest.mark.parametrize("shuffled", [False, True], ids=["listed", "shuffled"])
def test_one_call_over_mixed_frames(prod, eng, cases, shuffled, vector):
    """Frames that settle after 1, 5, 3, 2, 1 and 1 rounds in one call: the
    call takes the most any of them needs, and the rounds a frame does not
    need leave it alone."""
    names = list(MIXED)
    if shuffled:
        random.Random(7).shuffle(names)
        assert names != list(MIXED)
    cs = [cases[n] for n in names]
    bound = max(c.W for c in cs) + 1  # the call's mwg + 1
    rounds = [c.settled(bound).rounds for c in cs]
    assert rounds == [c.settled().rounds for c in cs]  # the call's larger bound changes nothing
    assert sorted(rounds) == [1, 1, 1, 2, 3, 5]
    n_max = max(c.n for c in cs)
    n_max += (n_max % 2 == 0) if not vector else 0
    assert decode_call(prod, eng, cs, n_max, vector) == max(rounds)


# ---------------------------------------------------------------- cmp_gpu_decode_stream
def test_through_decode_stream(prod, eng, cases):
    """The payloads of L2 and B1 as payload-only streams, the buffer behind
    them filled with 0xAB (which the model stages as the kernel does): the end
    check passes behind a DEC_BAD wave.  Then the control frame on the same
    engine."""
    import torch
    for name in ("L2", "B1"):
        c = cases[name]
        size, data = streams.oracle_stream(c.want, "u16", c.pre, c.enc, c.g, c.outlier)
        assert size == len(data) and data == c.payload and c.W == 3
        st = dm.Stream(data, 0, 8 * len(data), c.n, c.coder, tail=0xAB)
        r = dm.settle(st)
        assert r.rounds == 3 and not r.still_changed and r.exits[:-1] == r.true[1:]
        if name == "B1":
            assert r.handed_bad and set(r.fate.values()) == {"invalid"}
        else:
            assert set(r.fate.values()) == {"locked"} and len(r.wrong) >= 0.8 * (st.nsub - 1)
        host = np.full((len(data) + 7) // 8 * 8 + 64, 0xAB, dtype=np.uint8)
        host[:len(data)] = np.frombuffer(data, dtype=np.uint8)
        src = torch.from_numpy(host).cuda()
        dst = torch.full((c.n + GUARD,), FILL - 0x10000, dtype=torch.int16, device="cuda")
        status = torch.zeros(1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        with Launches(prod) as l:
            rc = eng.decode_stream(src.data_ptr(), len(data), c.n, c.pre, c.enc, c.g, c.outlier, dst.data_ptr(),
                                   status.data_ptr())
            assert eng.synchronize() == 0
        assert rc == 0, api.error_name(rc)
        s = int(status.cpu().numpy().astype(np.uint32)[0])
        assert s == c.n, (name, status_text(s))
        out = dst.cpu().numpy().view(np.uint16)
        assert np.array_equal(out[:c.n], c.want), name
        assert (out[c.n:] == FILL).all(), name
        assert l.delta[DECODE_ROUND] == r.rounds and sum(l.delta) == r.rounds, (name, l.named())
    assert decode_call(prod, eng, [cases["CTRL"]], cases["CTRL"].n, True) == 1


# ---------------------------------------------------------------- codeword ladder
@pytest.fixture(scope="module")
def ladder(orc, orc_ext):
    return [sc.ladder_case(orc, orc_ext, *coder) for coder in sc.ladder_coders()]


def test_codeword_ladder(prod, eng, ladder):
    """Every coder of the ladder (ZERO and MULTI, g from 1 to 65535, four
    outliers) over the values at which its codeword changes shape, each at
    every bit phase, the longest across a subsequence edge and one across the
    span edge (settle_cases.check_ladder); all frames in one call per store
    path.  No round count here."""
    assert len(ladder) == 13 + 13 * 4
    for c in ladder:
        sc.check_ladder(c)
    # coders whose every codeword has an even length reach the 16 even phases only
    assert sorted((c.g, c.outlier) for c in ladder if c.step == 2) == \
        [(32, 1), (32, 24), (33, 1), (32768, 1), (32768, 24), (32768, 107)]
    assert all(c.n == sc.LADDER_N for c in ladder)
    decode_call(prod, eng, ladder, sc.LADDER_N, True)
    decode_call(prod, eng, ladder, sc.LADDER_N + 1, False)
