"""The inputs of the decoder's settle tests (test_gpu_decode_settle.py on the
GPU, test_decode_model.py on the CPU): valid frames from the oracle's encoder
whose guessed parse starts are wrong, each anchored against the oracle and run
through the host model (decode_model.py) once per session."""
import functools

import numpy as np

import decode_model as dm
from conftest import load_pkg

api = load_pkg().cmpapi
HDR = 22  # bytes of a Golomb frame's header


def low16(x):
    return (np.asarray(x).astype(np.int64) & 0xFFFF).astype(np.uint16)


def laplace(seed, n, scale=20.0):
    return np.round(np.random.default_rng(seed).laplace(0, scale, n)).astype(np.int64)


def zigzag(r):
    r = ((np.asarray(r, dtype=np.int64) + 32768) & 0xFFFF) - 32768  # int16 wrap
    return np.where(r >= 0, 2 * r, -2 * r - 1)


def zero32_bits(r):
    """bits of each residual under GOLOMB_ZERO g = 32 (outlier 543)"""
    m = zigzag(r)
    return np.where(m < 543, (m + 1) // 32 + 6, 22)


def unmap(m):
    """mapped values -> int64 samples (ZigZag undone)"""
    m = np.asarray(m, dtype=np.int64)
    return np.where(m & 1, -(m + 1) // 2, m // 2)


def b1_samples(n):
    """48 bits each under MULTI g = 1, outlier 24: escape level 7 (31 ones, a
    zero) and 16 raw bits that end in 11 and so run into the next codeword's
    ones: a parse begun at the wrong place meets more than 32 ones in a row"""
    d = np.random.default_rng(31).integers(1 << 14, (1 << 16) - 28, n) | 3
    return -(24 + d + 1) // 2


def p1_samples():
    """1.7 workgroups of noise, a constant-512 run of 0.6 workgroup across the
    edge between workgroups 1 and 2, one workgroup of noise"""
    a, b = laplace(41, 40000), laplace(42, 25000)
    na = int(np.searchsorted(np.cumsum(zero32_bits(a)), 1.7 * dm.SPAN_BITS))
    nb = int(np.searchsorted(np.cumsum(zero32_bits(b)), 1.0 * dm.SPAN_BITS))
    run = np.full(int(0.6 * dm.SPAN_BITS / 22), 512, dtype=np.int64)
    return np.concatenate([a[:na], run, b[:nb]])


def control_samples():
    """3.4 workgroups of Laplace noise under DIFF + ZERO g = 32, the suite's staple"""
    x = laplace(43, 70000)
    n = int(np.searchsorted(np.cumsum(zero32_bits(np.diff(x, prepend=0))), 3.4 * dm.SPAN_BITS))
    return x[:n]


NONE, DIFF = 0, 1
ZERO, MULTI = dm.GOLOMB_ZERO, dm.GOLOMB_MULTI
# name: (preprocessing, encoder, g, outlier parameter, samples, parse workgroups)
CASES = {
    "L1w1": (NONE, ZERO, 1, 0, lambda: np.full(7500, 8), 1),
    "L1w2": (NONE, ZERO, 1, 0, lambda: np.full(12000, 8), 2),
    "L1w5": (NONE, ZERO, 1, 0, lambda: np.full(34000, 8), 5),
    "L1a": (NONE, ZERO, 1, 0, lambda: np.full(7710, 8), 1),
    "L1b": (NONE, ZERO, 1, 0, lambda: np.full(7711, 8), 2),
    "L2": (NONE, ZERO, 32, 0, lambda: np.full(15000, 512), 3),
    "L3": (DIFF, ZERO, 32, 0, lambda: 512 * np.arange(15000) % 65536, 3),
    "L4w5": (NONE, MULTI, 10, 107, lambda: np.full(22000, 700), 5),
    "L4w2": (NONE, MULTI, 10, 107, lambda: np.full(7000, 700), 2),
    "L5": (NONE, MULTI, 1055, 107, lambda: np.full(18000, 9), 2),
    "B1": (NONE, MULTI, 1, 2**32 - 1, lambda: b1_samples(6900), 3),
    "P1": (NONE, ZERO, 32, 0, p1_samples, 4),
    "CTRL": (DIFF, ZERO, 32, 0, control_samples, 4),
    "ONE": (NONE, ZERO, 32, 0, lambda: np.array([-3]), 1),
}


def oracle_frame(orc, pre, enc, g, outlier, x):
    p = api.CmpParams(primary_preprocessing=pre, primary_encoder_type=enc, primary_encoder_param=g,
                      primary_encoder_outlier=outlier)
    ctx = api.CmpContext()
    assert not api.is_error(orc.initialise(ctx, p))
    cap = 26 + 6 * len(x) + 64
    dst = api.aligned_empty(cap)
    r = orc.compress_u16(ctx, dst, cap, x)
    assert not api.is_error(r), api.error_name(r)
    return bytes(dst[:r])


class Case:
    """One frame: the source's low 16 bits (want), the oracle's frame, its
    payload, the model's Stream over the frame and the true parse.  Anchored
    on construction: the model's summed codeword lengths are the oracle's size,
    its mapped values give back the source, and so does orc_decode."""

    def __init__(self, orc, orc_ext, name, pre, enc, g, outlier, x):
        self.name, self.pre, self.enc, self.g, self.outlier = name, pre, enc, g, outlier
        self.want = low16(x)
        self.n = self.want.size
        self.frame = oracle_frame(orc, pre, enc, g, outlier, self.want)
        self.payload = self.frame[HDR:]
        self.W = (len(self.payload) + dm.SPAN_BYTES - 1) // dm.SPAN_BYTES
        self.coder = dm.Coder(enc, g, outlier)
        self.stream = dm.Stream(self.frame, HDR, 8 * len(self.payload), self.n, self.coder)
        self.bounds, self.mapped = self.stream.true_parse()
        assert (self.bounds[-1] + 7) // 8 == len(self.payload), (name, self.bounds[-1], len(self.payload))
        assert [self.coder.length(m) for m in self.mapped] == list(np.diff(self.bounds)), name
        res = unmap(self.mapped)
        assert np.array_equal(low16(np.cumsum(res) if pre == DIFF else res), self.want), name
        out = np.zeros(self.n, dtype=np.uint16)
        fr = np.frombuffer(self.frame, dtype=np.uint8)
        assert orc_ext.orc_decode(fr.ctypes.data, fr.size, None, out.ctypes.data, self.n) == self.n, name
        assert np.array_equal(out, self.want), name

    @functools.lru_cache(maxsize=None)
    def settled(self, max_rounds=None, broken=None):
        return dm.settle(self.stream, max_rounds, broken)


_cases = {}


def case(orc, orc_ext, name):
    if name not in _cases:
        pre, enc, g, outlier, make, W = CASES[name]
        c = _cases[name] = Case(orc, orc_ext, name, pre, enc, g, outlier, make())
        assert c.W == W, (name, c.W, len(c.payload))
    return _cases[name]


def summary(c, r):
    """one row of DESIGN.md 3.4's table"""
    fates = [r.fate[s] for s in r.wrong]
    return dict(case=c.name, n=c.n, bytes=len(c.payload), W=c.W, subsequences=c.stream.nsub, wrong=len(r.wrong),
                locked=fates.count("locked"), invalid=fates.count("invalid"), sync=fates.count("sync"),
                first_wrong=r.wrong[0] if r.wrong else None, last_wrong=r.wrong[-1] if r.wrong else None,
                rounds=r.rounds)


# ---------------------------------------------------------------- the codeword ladder
LADDER_G = (1, 2, 3, 7, 8, 31, 32, 33, 1055, 4096, 32767, 32768, 65535)
LADDER_OUTLIERS = (1, 24, 107, 2**32 - 1)
LADDER_N = 12000


def ladder_coders():
    return [(ZERO, g, 0) for g in LADDER_G] + [(MULTI, g, o) for g in LADDER_G for o in LADDER_OUTLIERS]


def ladder_values(c):
    """The mapped values at which a coder's codeword changes shape: 0, around
    the cutoff and the outlier (ZERO codes m + 1), every MULTI escape level's
    least and greatest raw value, and 65535."""
    s = {0, 65535}
    shift = 1 if c.enc == ZERO else 0
    s |= {c.cutoff - 1 - shift, c.cutoff - shift, c.outlier - 1, c.outlier}
    if c.enc == MULTI:
        for lvl in range(16):
            s |= {c.outlier + (0 if lvl == 0 else 4 ** lvl), c.outlier + 4 ** (lvl + 1) - 1}
    return sorted(int(m) for m in s if 0 <= m <= 65535)


def all_lengths(c):
    """codeword bits of every mapped value 0 .. 65535 (Coder.length, vectorised)"""
    m = np.arange(65536, dtype=np.int64)

    def golomb(v):
        return np.where(v < c.cutoff, c.k + 1, c.k + 2 + (v - c.cutoff) // c.g)
    if c.enc == ZERO:
        return np.where(m < c.outlier, golomb(m + 1), c.k + 17)
    d = np.maximum(m - c.outlier, 0)
    lvl = sum((d >= 4 ** j).astype(np.int64) for j in range(1, 16))
    return np.where(m < c.outlier, golomb(m), golomb(c.outlier + lvl) + 2 * (lvl + 1))


def ladder_case(orc, orc_ext, enc, g, outlier):
    """LADDER_N samples drawn from the coder's value set with a fixed seed.
    Three things can keep such a frame from what check_ladder asks, and each is
    mended here, not excused there:
      the set's codewords are all of even length although the coder has odd
        ones: the least value with an odd codeword is drawn as well (shifter);
      a boundary falls exactly on the span's edge, so no codeword straddles it:
        the draw is repeated with the next seed (attempt);
      the frame does not pass one span: n grows by 4000 (no coder here needs it).
    Where every codeword of the coder is even (step 2: k + 1 even and nothing
    a 16-bit sample maps to reaches past the cutoff) only the 16 even phases
    exist, and check_ladder asks for those."""
    key = ("ladder", enc, g, outlier)
    if key in _cases:
        return _cases[key]
    c = dm.Coder(enc, g, outlier)
    lens = all_lengths(c)
    vals = ladder_values(c)
    assert [c.length(v) for v in vals] == [int(lens[v]) for v in vals]
    step = int(np.gcd.reduce(np.append(lens, 32)))
    shifter = None
    if np.gcd.reduce(np.append(lens[vals], 32)) != step:
        shifter = int(np.argmax(lens % 2 == 1))
    draw = np.array(vals + ([shifter] if shifter is not None else []), dtype=np.int64)
    n, attempt = LADDER_N, 0
    while True:
        rng = np.random.default_rng([enc, g, outlier & 0xFFFF, n, attempt])
        m = draw[rng.integers(0, draw.size, n)]
        ends = np.cumsum(lens[m])
        if ends[-1] <= dm.SPAN_BITS:
            n += 4000
        elif dm.SPAN_BITS in ends:
            attempt += 1
        else:
            break
    k = _cases[key] = Case(orc, orc_ext, f"ladder enc {enc} g {g} outlier {outlier}", NONE, enc, g, outlier, unmap(m))
    k.values, k.shifter, k.step, k.attempt, k.longest = vals, shifter, step, attempt, int(lens.max())
    return k


def check_ladder(c):
    """The frame exercises what it is for: every value of the coder's set starts
    at every bit phase of a word (all 32, or the 16 even ones where the coder
    has no codeword of odd length), a codeword of the coder's greatest length
    straddles a 512-bit edge, and one straddles the edge of the first
    workgroup's span."""
    assert c.n <= 70000 and c.bounds[-1] > dm.SPAN_BITS, (c.name, c.n, c.bounds[-1])
    assert c.step in (1, 2) and c.longest == max(c.coder.length(v) for v in c.values), c.name
    phases = {v: set() for v in c.values}
    over_sub = over_span = False
    for m, a, b in zip(c.mapped, c.bounds, c.bounds[1:]):
        if m != c.shifter or m in phases:
            phases[m].add((HDR * 8 + a) & 31)
        over_sub |= b - a == c.longest and a // dm.DEC_B != (b - 1) // dm.DEC_B
        over_span |= a < dm.SPAN_BITS < b
    short = {v: len(p) for v, p in phases.items() if len(p) != 32 // c.step}
    assert not short, (c.name, short)
    assert over_sub and over_span, (c.name, c.longest, over_sub, over_span)


# ---------------------------------------------------------------- what each case is for
LOCKED = ("L1w1", "L1w2", "L1w5", "L1a", "L1b", "L2", "L3", "L4w5", "L4w2", "L5")


def check_property(c, r):
    """The model's result has the property the case stands for, so that a case
    cannot quietly stop exercising its path (r: settled with the default bound)."""
    name, nsub = c.name, c.stream.nsub
    fates = [r.fate[s] for s in r.wrong]
    assert not r.still_changed, name
    if name in LOCKED:
        # wrong guesses stay wrong: every round hands the truth one workgroup on
        assert len(r.wrong) >= 0.8 * (nsub - 1), (name, len(r.wrong), nsub)
        assert "sync" not in fates, name
        if name == "L5":
            assert "invalid" in fates and "locked" in fates, name
        else:
            assert set(fates) == {"locked"} and dm.DEC_BAD not in r.first_exits, name
        assert r.rounds == c.W, (name, r.rounds)
        assert [bool(m) for m in r.moved] == [True] * (c.W - 1) + [False], (name, r.moved)  # every round but the last
    elif name == "B1":
        assert len(c.payload) == 6 * c.n
        assert 2 * len(r.wrong) > nsub and set(fates) == {"invalid"}, (name, len(r.wrong))
        assert r.handed_bad and r.rounds == c.W == 3, (name, r.handed_bad, r.rounds)
    elif name == "P1":
        wg = 2  # the workgroup behind the edge the constant run crosses
        o0, hi = wg * dm.DEC_WG, (wg + 1) * dm.DEC_WG
        assert o0 in r.wrong and o0 - 1 in r.wrong, name
        assert r.first_exits[hi - 1] == r.exits[hi - 1] == r.true[hi], name
        assert r.rounds == 1 and r.redone == [[wg]] and r.moved == [[]], (name, r.redone, r.moved)
        assert r.first_wg_cnt[wg] != r.wg_cnt[wg], name  # the redo changes the count the scan needs
        assert r.first_wg_cnt[wg + 1] == r.wg_cnt[wg + 1], name
    else:  # CTRL, ONE
        assert not r.wrong and r.rounds == 1 and r.redone == [[]], name
    assert r.wg_cnt == [sum(r.cnt[w * dm.DEC_WG:(w + 1) * dm.DEC_WG]) for w in range(c.stream.nwg)]
    assert r.exits[:-1] == r.true[1:] and sum(r.wg_cnt) >= c.n, name
