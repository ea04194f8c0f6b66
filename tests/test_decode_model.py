"""The host model of the decoder's parser (decode_model.py) and the inputs of
test_gpu_decode_settle.py (settle_cases.py), checked without a GPU: the
model's codewords against a restated encoder, every case anchored against the
oracle and holding the property it stands for, the figures DESIGN.md 3.4
quotes, and the model's own view of three deliberate defects of the kernel."""
import random

import numpy as np
import pytest

import decode_model as dm
import settle_cases as sc


def put(c, m):
    """(bits, length) the encoder writes for mapped value m (encoder.c:303-378)"""
    def golomb(v):
        if v < c.cutoff:
            return v, c.k + 1
        q, r = divmod(v - c.cutoff, c.g)
        return (((1 << q) - 1) << (c.k + 2)) | (2 * c.cutoff + r), c.k + 2 + q
    if c.enc == dm.GOLOMB_ZERO:
        return golomb(m + 1) if m < c.outlier else (m, c.k + 17)
    if m < c.outlier:
        return golomb(m)
    d = m - c.outlier
    lvl = 0 if d < 4 else (d.bit_length() - 1) // 2
    v, ln = golomb(c.outlier + lvl)
    return (v << 2 * (lvl + 1)) | d, ln + 2 * (lvl + 1)


@pytest.mark.parametrize("enc,g,outlier", sc.ladder_coders())
def test_codeword_inverts_the_encoder(enc, g, outlier):
    """window_codeword reads back what the encoder writes, whatever follows it
    in the window; the lengths are Coder.length's and all_lengths'; no
    codeword passes 48 bits (the Golomb part 32)."""
    c = dm.Coder(enc, g, outlier)
    rng = random.Random(g * 7 + enc)
    lens = sc.all_lengths(c)
    assert lens.max() <= 48
    for m in sc.ladder_values(c) + [rng.randrange(65536) for _ in range(200)]:
        v, ln = put(c, m)
        assert ln == c.length(m) == lens[m] and v < (1 << ln)
        for fill in (0, (1 << (64 - ln)) - 1, rng.getrandbits(64 - ln)):
            assert dm.window_codeword(c, (v << (64 - ln)) | fill) == (ln, m), (m, ln, fill)


def test_invalid_codewords():
    c = dm.Coder(dm.GOLOMB_MULTI, 1, 2**32 - 1)
    assert (c.cutoff, c.outlier) == (1, 24)
    ones = lambda q: ((1 << q) - 1) << (64 - q)  # noqa: E731
    assert dm.window_codeword(c, ones(33))[0] == 0  # more than 32 ones
    assert dm.window_codeword(c, ones(31)) == (48, 24)  # level 7, raw bits 0
    assert dm.window_codeword(c, ones(32))[0] == 0  # level 8: 33 + 18 bits
    z = dm.Coder(dm.GOLOMB_ZERO, 1)
    assert (z.cutoff, z.outlier) == (1, 16)
    assert dm.window_codeword(z, 16 << 47) == (17, 16)  # sample 8: a zero, 16 raw bits
    assert dm.window_codeword(z, ones(32)) == (33, 31) and dm.window_codeword(z, ones(33))[0] == 0


@pytest.mark.parametrize("name", list(sc.CASES))
def test_case_is_anchored_and_holds_its_property(orc, orc_ext, name):
    c = sc.case(orc, orc_ext, name)  # anchored on construction (settle_cases.Case)
    r = c.settled()
    sc.check_property(c, r)
    # the model's own scan and output pass give back the source
    res = np.array(dm.decoded(c.stream, r), dtype=np.int64)
    assert np.array_equal(sc.low16(np.cumsum(res) if c.pre == sc.DIFF else res), c.want)


# case: (subsequences, wrong guesses, of them locked, invalid, in step again, rounds): DESIGN.md 3.4
TABLE = {
    "CTRL": (871, 0, 0, 0, 0, 1),
    "L1w5": (1129, 1062, 1062, 0, 0, 5),
    "L2": (645, 586, 586, 0, 0, 3),
    "L3": (645, 586, 586, 0, 0, 3),
    "L4w5": (1161, 1074, 1074, 0, 0, 5),
    "L5": (387, 316, 211, 105, 0, 2),
    "B1": (647, 431, 0, 431, 0, 3),
    "P1": (845, 153, 0, 0, 153, 1),
}


@pytest.mark.parametrize("name", list(TABLE))
def test_design_table(orc, orc_ext, name):
    c = sc.case(orc, orc_ext, name)
    s = sc.summary(c, c.settled())
    assert (s["subsequences"], s["wrong"], s["locked"], s["invalid"], s["sync"], s["rounds"]) == TABLE[name], s


# what the model makes of each defect: "rounds" another round count, "samples"
# other samples, "status" fewer than n codewords found (INT_BITSTREAM)
BREAKS = {
    "no_redo": {"L1w2": "rounds samples", "L1w5": "rounds samples", "L2": "rounds samples", "L3": "rounds samples",
                "L4w5": "rounds samples", "L4w2": "rounds samples", "L5": "rounds samples", "B1": "rounds status",
                "P1": "samples"},
    "no_changed": {"L1w2": "rounds", "L1w5": "rounds samples", "L1b": "rounds", "L2": "rounds samples",
                   "L3": "rounds samples", "L4w5": "rounds samples", "L4w2": "rounds", "L5": "rounds",
                   "B1": "rounds status"},
}
BREAKS["one_round"] = BREAKS["no_changed"]


@pytest.mark.parametrize("broken", list(BREAKS))
def test_model_tells_the_defects_apart(orc, orc_ext, broken):
    """The model with one of three defects of decode.hip built in (settle's
    broken=) disagrees with its unbroken self on the cases that are there to
    catch it, and on no other."""
    seen = {}
    for name in sc.CASES:
        c = sc.case(orc, orc_ext, name)
        good, bad = c.settled(), c.settled(None, broken)
        want, got = dm.decoded(c.stream, good), dm.decoded(c.stream, bad)
        what = ["rounds"] if bad.rounds != good.rounds else []
        if got != want:
            what.append("status" if got is None else "samples")
        if what:
            seen[name] = " ".join(what)
    assert seen == BREAKS[broken]


def test_ladder_frames(orc, orc_ext):
    """every ladder frame is anchored and exercises what check_ladder asks"""
    for coder in sc.ladder_coders():
        sc.check_ladder(sc.ladder_case(orc, orc_ext, *coder))


def test_launch_stats_serve_a_caller_that_knows_fewer_counters(prod):
    """airs_dev_launch_stats returns how many counters it copied: the six a
    caller from before AIRS_STAT_DECODE_ROUND asks for, the seven one from
    before the walk and fallback-step counters asks for, never more than the
    library has, and nothing behind them in the caller's array."""
    import ctypes
    from rice_helpers import STAT_NAMES
    fn = prod.lib.airs_dev_launch_stats
    fn.argtypes = [ctypes.POINTER(ctypes.c_uint64), ctypes.c_uint32]
    fn.restype = ctypes.c_uint32
    have = len(STAT_NAMES)
    assert have == 10
    for n in (0, 1, 6, 7, have, have + 5):
        out = (ctypes.c_uint64 * (have + 6))(*([2**64 - 1] * (have + 6)))
        got = fn(out, n)
        assert got == min(n, have), (n, got)
        assert all(v == 2**64 - 1 for v in list(out)[got:]), n
