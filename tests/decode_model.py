"""A host model of the GPU decoder's speculative parse (csrc/decode.hip), for
the tests only: plain Python integers, nothing of the library.

It restates three things of the decoder:
  codeword   one codeword's length and mapped value at a bit position
             (dec_window), with the encoder's own resolution of cutoff and
             outlier (encoder.c:185-224);
  guesses    where a subsequence's parse begins when nothing is known
             (warm_start: DEC_WARM bits earlier, the first boundary at or past
             the subsequence);
  rounds     parse_wg's rounds as decode_frames drives them: the speculative
             launch settles every workgroup from its first guess, each later
             launch hands a workgroup the last exit its predecessor had one
             launch earlier, skips it when that start did not move, and the
             host stops at the first launch after which no workgroup's last
             exit moved.

The settle loop inside a workgroup is a Jacobi iteration whose fixed point is
unique (thread t starts where thread t - 1 stopped), so the model chains the
threads sequentially.  Bits past the payload are what the kernel stages: the
frame's bytes up to the next 4-byte word (`tail` bytes of the caller's buffer),
then the last word again (stage_span clamps the word index).

settle(..., broken=...) restates three deliberate defects of the kernel, so a
test can show that the model tells them apart:
  "no_redo"     rounds past the first redo thread 0 only (the t != 0 branch
                keeps exit_in, cnt and base whatever its start became)
  "no_changed"  *a.changed is never set
  "one_round"   the host loop stops after its first launch
"""
DEC_B = 512      # bits per subsequence
DEC_WG = 256     # subsequences per workgroup
DEC_WARM = 192   # bits decoded before a guessed start
DEC_BAD = 0xFFFFFFFF
SPAN_BITS = DEC_WG * DEC_B
SPAN_BYTES = SPAN_BITS // 8

UNCOMPRESSED, GOLOMB_ZERO, GOLOMB_MULTI = 0, 1, 2
M64 = (1 << 64) - 1


class Coder:
    """Encoder type and Golomb parameter with cutoff and outlier resolved as the
    encoder resolves them: the outlier is capped at the first value whose
    codeword would pass 32 bits, 8 earlier for MULTI (its escape symbols);
    ZERO derives its own outlier from the parameter."""

    def __init__(self, enc, g=1, outlier=0):
        self.enc, self.g = enc, g
        self.k = self.cutoff = self.outlier = 0
        if enc == UNCOMPRESSED:
            return
        assert enc in (GOLOMB_ZERO, GOLOMB_MULTI) and 1 <= g <= 0xFFFF
        self.k = g.bit_length() - 1
        self.cutoff = (2 << self.k) - g
        limit = self.cutoff + (31 - self.k) * g
        if enc == GOLOMB_MULTI:
            limit = max(limit - 8, 0)
            want = outlier
        else:
            want = min(self.cutoff + 16 * g - 1, 0xFFFFFFFF)
        self.outlier = min(want, limit)
        assert self.outlier > 0

    def golomb_len(self, v):
        """bits of the Golomb codeword of v (encoder.c:303-324)"""
        if v < self.cutoff:
            return self.k + 1
        return self.k + 2 + (v - self.cutoff) // self.g

    def length(self, m):
        """bits the encoder spends on mapped value m (encoder.c:327-378)"""
        if self.enc == UNCOMPRESSED:
            return 16
        if self.enc == GOLOMB_ZERO:
            return self.golomb_len(m + 1) if m < self.outlier else self.k + 17
        if m < self.outlier:
            return self.golomb_len(m)
        d = m - self.outlier
        lvl = 0 if d < 4 else (d.bit_length() - 1) // 2
        return self.golomb_len(self.outlier + lvl) + 2 * (lvl + 1)


def window_codeword(c, W):
    """One codeword at the top of the 64-bit window W: (length, mapped value);
    length 0 is an invalid codeword: more than 32 leading ones, an escape
    level over 15 or more than 48 bits."""
    if c.enc == UNCOMPRESSED:
        return 16, W >> 48
    q = 0
    while q < 64 and (W >> (63 - q)) & 1:
        q += 1
    if q > 32:
        return 0, None
    rest = (W << (q + 1)) & M64
    x = rest >> (64 - c.k) if c.k else 0
    ln = q + 1 + c.k
    if x >= c.cutoff:
        x = ((x << 1) | (((rest << c.k) & M64) >> 63)) - c.cutoff
        ln += 1
    u = q * c.g + x
    if c.enc == GOLOMB_ZERO:
        if u == 0:
            m = ((W << ln) & M64) >> 48
            ln += 16
        else:
            m = u - 1
    elif u < c.outlier:
        m = u
    else:
        lvl = u - c.outlier
        if lvl > 15:
            return 0, None
        nb = 2 * (lvl + 1)
        if ln + nb > 64:
            return 0, None
        m = c.outlier + (((W << ln) & M64) >> (64 - nb))
        ln += nb
    return (0, None) if ln > 48 else (ln, m)


def unmap(c, m):
    """mapped value -> the 16-bit residual"""
    return m & 0xFFFF if c.enc == UNCOMPRESSED else ((m >> 1) ^ -(m & 1)) & 0xFFFF


class Stream:
    """A frame's payload (data[hdr_bytes : hdr_bytes + nbits / 8]) or a
    payload-only stream (hdr_bytes = 0) as the kernel stages it; n codewords."""

    def __init__(self, data, hdr_bytes, nbits, n, coder, tail=0):
        self.c, self.n, self.nbits, self.hdr_bits = coder, n, nbits, 8 * hdr_bytes
        words = (len(data) + 3) // 4
        buf = bytes(data) + bytes([tail]) * (4 * words - len(data))
        self.buf = buf + buf[-4:] * 4  # stage_span clamps the word index to the frame's last word
        self.nsub = (nbits + DEC_B - 1) // DEC_B if n else 0
        self.nwg = (self.nsub + DEC_WG - 1) // DEC_WG
        self._cw, self._pr = {}, {}

    def codeword(self, pos):
        r = self._cw.get(pos)
        if r is None:
            a = self.hdr_bits + pos
            w = int.from_bytes(self.buf[a >> 3:(a >> 3) + 9], "big")
            r = self._cw[pos] = window_codeword(self.c, (w >> (8 - (a & 7))) & M64)
        return r

    def end(self, s):
        return min((s + 1) * DEC_B, self.nbits)

    def parse_range(self, start, end):
        """(exit, codewords) of a parse of [start, end); an invalid codeword
        ends it at DEC_BAD with the codewords before it counted"""
        if start == DEC_BAD:
            return DEC_BAD, 0
        r = self._pr.get((start, end))
        if r is None:
            p, cnt = start, 0
            while p < end:
                ln = self.codeword(p)[0]
                if not ln:
                    p = DEC_BAD
                    break
                p += ln
                cnt += 1
            r = self._pr[(start, end)] = (p, cnt)
        return r

    def warm_start(self, r0):
        p = r0 - min(r0, DEC_WARM)
        while p < r0:
            ln = self.codeword(p)[0]
            if not ln:
                return r0
            p += ln
        return p

    def true_parse(self):
        """the n codewords from bit 0: (boundaries [n + 1], mapped values [n])"""
        b, ms, p = [0], [], 0
        for _ in range(self.n):
            ln, m = self.codeword(p)
            assert ln, f"invalid codeword at bit {p} of a valid stream"
            p += ln
            b.append(p)
            ms.append(m)
        return b, ms

    def chain(self, wg, in_start):
        """workgroup wg settled from in_start: (starts, exits, counts) of its live threads"""
        starts, exits, cnts, st = [], [], [], in_start
        for s in range(wg * DEC_WG, min((wg + 1) * DEC_WG, self.nsub)):
            ex, c = self.parse_range(st, self.end(s))
            starts.append(st)
            exits.append(ex)
            cnts.append(c)
            st = ex
        return starts, exits, cnts


class Settled:
    """What settle() found.
    guess[s]   subsequence s's guessed start (0 for s = 0)
    true[s]    where its parse really begins (the chain from bit 0)
    wrong      the subsequences whose guess is not that
    fate[s]    for a wrong guess, what a parse begun there does when it just goes
               on: "sync" (meets a true boundary), "invalid" (meets an invalid
               codeword first) or "locked" (neither before the payload ends)
    rounds     launches of dec_parse_kernel with first == 0, the last one that
               reports no change included
    redone[r]  the workgroups round r + 1 did not skip
    moved[r]   the workgroups whose last exit round r + 1 changed
    handed_bad (round, workgroup) of every redo that began at DEC_BAD
    first_exits, first_wg_cnt  exits and workgroup counts after the speculative launch
    still_changed  the host loop ran out of rounds while a last exit still moved
    base, exits, cnt, wg_cnt   the arrays as the last launch left them"""


def settle(st, max_rounds=None, broken=None):
    """Runs the launches of decode_frames over one stream.  max_rounds: the
    call's bound, mwg + 1 of the call's largest frame (default: this one)."""
    r = Settled()
    nsub, nwg = st.nsub, st.nwg
    r.guess = [0] + [st.warm_start(s * DEC_B) for s in range(1, nsub)]
    base, exits, cnt, wg_cnt = [], [], [], []
    for wg in range(nwg):  # the speculative launch: each workgroup settles from its first guess
        a, b, c = st.chain(wg, r.guess[wg * DEC_WG])
        base += a
        exits += b
        cnt += c
        wg_cnt.append(sum(c))
    r.first_exits, r.first_wg_cnt = list(exits), list(wg_cnt)
    r.rounds, r.redone, r.moved, r.handed_bad = 0, [], [], []
    bound = (nwg + 1) if max_rounds is None else max_rounds
    while nsub and r.rounds < bound:
        prev, changed, redone, moved = list(exits), False, [], []
        for wg in range(nwg):
            o0 = wg * DEC_WG
            hi = min(o0 + DEC_WG, nsub)
            in_start = 0 if wg == 0 else prev[o0 - 1]
            if base[o0] == in_start:
                continue
            redone.append(wg)
            if in_start == DEC_BAD:
                r.handed_bad.append((r.rounds + 1, wg))
            if broken == "no_redo":
                base[o0] = in_start
                exits[o0], cnt[o0] = st.parse_range(in_start, st.end(o0))
            else:
                base[o0:hi], exits[o0:hi], cnt[o0:hi] = st.chain(wg, in_start)
            wg_cnt[wg] = sum(cnt[o0:hi])
            if exits[hi - 1] != prev[hi - 1]:
                moved.append(wg)
                changed = broken != "no_changed"
        r.rounds += 1
        r.redone.append(redone)
        r.moved.append(moved)
        if not changed or broken == "one_round":
            break
    r.still_changed = bool(nsub) and changed
    r.base, r.exits, r.cnt, r.wg_cnt = base, exits, cnt, wg_cnt
    # the truth: one chain from bit 0
    r.true, p = [], 0
    for s in range(nsub):
        r.true.append(p)
        p = st.parse_range(p, st.end(s))[0]
    r.wrong = [s for s in range(nsub) if r.guess[s] != r.true[s]]
    bounds = set(st.true_parse()[0])
    fate = {}
    for s in r.wrong:
        path, p = [], r.guess[s]
        while True:
            if p in fate:
                f = fate[p]
                break
            if p in bounds:
                f = "sync"
                break
            if p >= st.nbits:
                f = "locked"
                break
            ln = st.codeword(p)[0]
            if not ln:
                f = "invalid"
                break
            path.append(p)
            p += ln
        for q in path:
            fate[q] = f
        fate[r.guess[s]] = f
    r.fate = {s: fate[r.guess[s]] for s in r.wrong}
    return r


def decoded(st, r):
    """The residuals dec_scan_kernel and dec_out_kernel make of a settled state
    (None where the scan finds fewer than n codewords: INT_BITSTREAM): every
    subsequence decodes from its predecessor's exit and writes from the
    exclusive sum of the counts before it."""
    if sum(r.wg_cnt) < st.n:
        return None
    out = [None] * st.n
    for wg in range(st.nwg):
        j = sum(r.wg_cnt[:wg])
        for s in range(wg * DEC_WG, min((wg + 1) * DEC_WG, st.nsub)):
            p, i = (r.exits[s - 1] if s else 0), j
            while p < st.end(s) and i < st.n and p != DEC_BAD:
                ln, m = st.codeword(p)
                if not ln:
                    break
                p += ln
                out[i] = unmap(st.c, m)
                i += 1
            j += r.cnt[s]
    return out
