"""cmp_gpu_compress_image with CMP_GPU_OPT_IMAGE_RAGGED and
CMP_GPU_OPT_IMAGE_RAGGED_CHECKSUM: checksum-enabled contexts in ragged pieces
(checksum.hip, enc_ragged.hip).  The options change the
schedule only, so truth is what it is without them: the CPU oracle's call loop
over the same table (tests/encode_image_helpers.py `truth`, which honours
checksum_enabled).  After every call the sizes, the offsets, the image bytes,
the guards and the context's fields are compared (eh.same); the device layer's
counters (airs_dev_ragged_stats, airs_dev_ragged_ck_stats,
airs_dev_launch_stats) say which way the frames went.

S below is the ragged kernel's segment in samples (airs_dev_ragged_segment).
The XXH32 consumes stripes of 8 samples, the chain kernel reads them in round
quads (32 samples) and looks 128 rounds (1024 samples) ahead; the product
kernel's workgroups take 256 quads (8192 samples) each."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import encode_image_helpers as eh
from conftest import PKG_DIR, load_pkg

pytestmark = pytest.mark.gpu
pkg = load_pkg()
api = pkg.cmpapi
P = api.CmpParams
CLI = os.path.join(PKG_DIR, "bin", "airspace")

ZERO32 = dict(primary_preprocessing=eh.DIFF, primary_encoder_type=eh.GOLOMB_ZERO, primary_encoder_param=32)
CK = dict(checksum_enabled=1, **ZERO32)
MIXED = [0, 5, 2, 11, 14, 7]  # byte phases of the frames in the sample image


@pytest.fixture(scope="module")
def eng(prod):
    """These tests' own engine; every test sets the options it needs."""
    if not prod.gpu_available():
        pytest.fail("GPU test run without a usable HIP device")
    e = prod.engine()
    yield e
    e.close()


@pytest.fixture
def both(eng):
    assert eng.set_option(pkg.OPT_IMAGE_RAGGED, 1) == 0
    assert eng.set_option(pkg.OPT_IMAGE_RAGGED_CHECKSUM, 1) == 0
    assert eng.set_option(pkg.OPT_IMAGE_CHUNK, 0) == 0
    yield eng
    assert eng.set_option(pkg.OPT_IMAGE_RAGGED, 0) == 0
    assert eng.set_option(pkg.OPT_IMAGE_RAGGED_CHECKSUM, 0) == 0
    assert eng.set_option(pkg.OPT_IMAGE_CHUNK, 0) == 0


def counters(prod, name, count):
    out = (ctypes.c_uint64 * count)()
    fn = getattr(prod.lib, name)
    fn.argtypes, fn.restype = [ctypes.c_void_p, ctypes.c_uint32], ctypes.c_uint32
    assert fn(out, count) == count
    return [int(v) for v in out]


class Moved:
    """What the counters moved by between two points of a test."""

    def __init__(self, prod):
        self.prod = prod
        self.at = self.read()

    def read(self):
        return (counters(self.prod, "airs_dev_ragged_stats", 3), counters(self.prod, "airs_dev_ragged_ck_stats", 2),
                eh.stage_frames(self.prod), counters(self.prod, "airs_dev_launch_stats", 10))

    def take(self):
        now = self.read()
        d = [[a - b for a, b in zip(n, o)] for n, o in zip(now, self.at)]
        self.at = now
        self.launches, self.frames, self.blocks = d[0]
        self.ck_launches, self.ck_frames = d[1]
        self.ingested, self.emitted, self.refused = d[2]
        self.batch = sum(d[3])
        return self


def segment(prod, kind):
    fn = prod.lib.airs_dev_ragged_segment
    fn.argtypes, fn.restype = [ctypes.c_uint32], ctypes.c_uint32
    return int(fn(eh.sample_bytes(kind)))


def walk(rng, n, step=12):
    """A random walk with outliers: it compresses, and some samples escape."""
    x = 30000 + np.cumsum(rng.integers(-step, step + 1, n))
    hit = rng.random(n) < 0.01
    x = x + hit * rng.integers(-30000, 30000, n)
    return (x & 0xFFFF).astype(np.uint16)


def in_i32(rng, x):
    """16-bit samples in 32-bit words with junk upper halves, which neither
    the encoder nor the checksum may see."""
    junk = rng.integers(0, 1 << 16, x.size).astype(np.uint32) << 16
    return (junk | x.astype(np.uint32)).view(np.uint8)


def check(prod, eng, orc, params, kind, img, offs, fbs, what="", **kw):
    t = eh.truth(orc, params, kind, img, offs, fbs, big_endian=kw.get("big_endian", False))
    g = eh.run(prod, eng, params, kind, img, offs, fbs, total=t.offsets[-1], **kw)
    eh.same(g, t, what)
    return g, t


def frames_of(r):
    return [r.image[o:o + s] for o, s in zip(r.offsets, r.sizes)]


def checksum_bits(r):
    return [f[15] >> 3 & 1 for f in frames_of(r)]


# ---------------------------------------------------------------- 1. checksum loop edges
LOOP_NS = [1, 2, 3, 4, 7, 8, 9, 15, 16, 17, 31, 32, 33, 1016, 1023, 1024, 1025, 1031, 1032, 1033, 2047, 2048, 2056]
FORMS = {
    "u16-aligned": ("u16", [0]),
    "u16-even-unaligned": ("u16", [2, 4, 6, 10, 14, 8, 12]),
    "i16-in-i32-junk": ("i16_in_i32", [0, 4, 8, 12]),
}


@pytest.mark.parametrize("form", sorted(FORMS))
def test_checksum_loop_edges_in_one_piece(prod, both, orc, form):
    """No stripe (under 8 samples), tails of every length, one and several
    round quads, the look-ahead batch of 128 rounds (1024 samples) with its
    remainder; 4-byte samples at phases 4 and 12 take the product kernel's
    sample-by-sample path as the unaligned u16 frames do."""
    kind, phases = FORMS[form]
    rng = np.random.default_rng(11)
    chunks = [in_i32(rng, walk(rng, n)) if kind == "i16_in_i32" else eh.stored(walk(rng, n), False) for n in LOOP_NS]
    img, offs = eh.place(chunks, phases)
    if form == "u16-aligned":
        assert all(o % 16 == 0 for o in offs)
    if form == "u16-even-unaligned":
        assert all(o % 2 == 0 and o % 16 for o in offs)
    m = Moved(prod)
    g, t = check(prod, both, orc, P(**CK), kind, img, offs, [len(c) for c in chunks], what=form, out_phase=3)
    m.take()
    assert (m.launches, m.frames, m.batch) == (1, len(LOOP_NS), 0)
    assert (m.ck_launches, m.ck_frames) == (1, len(LOOP_NS))
    assert m.ingested == 0  # every frame is read where it lies, by the checksum too
    assert checksum_bits(g) == [1] * len(LOOP_NS)


# ---------------------------------------------------------------- 2. segment edges
@pytest.mark.parametrize("kind", ["u16", "i16_in_i32"])
def test_segment_edges_under_a_checksum(prod, both, orc, kind):
    """The checksum follows a last segment that is full (S, the only one),
    nearly empty (S + 1, 2 S + 9) or nearly full (S - 1)."""
    S = segment(prod, kind)
    rng = np.random.default_rng(22)
    ns = [S - 1, 3, S, 5, S + 1, 1, 2 * S + 9]
    chunks = [in_i32(rng, walk(rng, n)) if kind == "i16_in_i32" else eh.stored(walk(rng, n), False) for n in ns]
    img, offs = eh.place(chunks, [0, 4, 8])
    m = Moved(prod)
    check(prod, both, orc, P(**CK), kind, img, offs, [len(c) for c in chunks], what=kind, out_phase=1)
    m.take()
    assert (m.launches, m.frames, m.blocks) == (1, len(ns), sum(-(-n // S) for n in ns))
    assert (m.ck_launches, m.ck_frames) == (1, len(ns))


# ---------------------------------------------------------------- 3. chain groups
def group_table(rng, count):
    """Mixed sizes under 100 samples and around the stripe and quad edges."""
    pool = [1, 5, 8, 13, 31, 32, 33, 64, 77, 99, 200, 1030, 7, 16, 2, 40]
    return [pool[(3 * i + count) % len(pool)] + int(rng.integers(0, 3)) for i in range(count)]


@pytest.mark.parametrize("count", [1, 15, 16, 17, 33])
def test_chain_groups(prod, both, orc, count):
    """A chain wave holds sixteen frames: tables that leave slots of the last
    wave empty, fill it exactly and start another."""
    rng = np.random.default_rng(33 + count)
    ns = group_table(rng, count)
    img, offs = eh.place([eh.stored(walk(rng, n), False) for n in ns], [0, 2, 6])
    m = Moved(prod)
    g, t = check(prod, both, orc, P(**CK), "u16", img, offs, [2 * n for n in ns], what=count)
    m.take()
    assert (m.ck_launches, m.ck_frames, m.launches) == (1, count, 1)
    # the checksums land at their frames: the last four bytes of each, against the loop's
    assert [f[-4:] for f in frames_of(g)] == [f[-4:] for f in t.frames]
    assert len({f[-4:] for f in t.frames}) == count


def test_one_long_frame_among_short_ones(prod, both, orc):
    """One wave's slots differ widely: about 40 000 samples beside frames of
    under 100, in the middle of a group of sixteen and of a table of 21."""
    rng = np.random.default_rng(34)
    ns = [int(v) for v in rng.integers(1, 100, 21)]
    ns[9] = 40003
    img, offs = eh.place([eh.stored(walk(rng, n), False) for n in ns], [0, 2, 6, 12])
    m = Moved(prod)
    g, t = check(prod, both, orc, P(**CK), "u16", img, offs, [2 * n for n in ns])
    m.take()
    assert (m.ck_launches, m.ck_frames, m.launches, m.batch) == (1, 21, 1, 0)
    assert [f[-4:] for f in frames_of(g)] == [f[-4:] for f in t.frames]


# ---------------------------------------------------------------- 4. staged and direct frames
def test_staged_and_direct_frames_in_one_piece(prod, both, orc):
    """Native u16 at odd byte addresses is staged and the checksum reads the
    row; the same table from an odd address swaps the two sets; a big-endian
    table stages every frame."""
    rng = np.random.default_rng(44)
    ns = [1000, 1001, 5000, 16385, 37, 1002, 20000, 999, 7]
    phases = [0, 1, 6, 3, 10, 14, 5, 2, 9]
    xs = [walk(rng, n) for n in ns]
    fbs = [2 * n for n in ns]
    img, offs = eh.place([eh.stored(x, False) for x in xs], phases)
    odd = sum(o % 2 for o in offs)
    assert 0 < odd < len(ns)
    m = Moved(prod)
    check(prod, both, orc, P(**CK), "u16", img, offs, fbs)
    m.take()
    assert (m.launches, m.ck_launches, m.ck_frames, m.ingested) == (1, 1, len(ns), odd)
    check(prod, both, orc, P(**CK), "u16", img, offs, fbs, src_phase=1)
    m.take()
    assert (m.launches, m.ck_launches, m.ck_frames, m.ingested) == (1, 1, len(ns), len(ns) - odd)
    img, offs = eh.place([eh.stored(x, True) for x in xs], MIXED)
    check(prod, both, orc, P(**CK), "u16", img, offs, fbs, big_endian=True, out_phase=5)
    m.take()
    assert (m.launches, m.ck_launches, m.ck_frames, m.ingested) == (1, 1, len(ns), len(ns))


# ---------------------------------------------------------------- 5. every coder
def coder(pre, enc, g=0, outlier=0):
    return P(primary_preprocessing=pre, primary_encoder_type=enc, primary_encoder_param=g,
             primary_encoder_outlier=outlier, checksum_enabled=1)


CODERS = {
    "none-raw": coder(eh.NONE, eh.UNCOMPRESSED),
    "diff-zero32": coder(eh.DIFF, eh.GOLOMB_ZERO, 32),
    "diff-zero3": coder(eh.DIFF, eh.GOLOMB_ZERO, 3),
    "diff-multi7": coder(eh.DIFF, eh.GOLOMB_MULTI, 7, 40),
}


@pytest.fixture(scope="module")
def coder_table(prod):
    rng = np.random.default_rng(55)
    S = segment(prod, "i16")
    ns = [1, 9, 16, 17, 4095, 4097, S - 1, S, S + 1, 2 * S + 5, 33]
    img, offs = eh.place([eh.stored(walk(rng, n), False) for n in ns], [0, 3, 2, 14, 9])
    return img, offs, [2 * n for n in ns]


@pytest.mark.parametrize("name", sorted(CODERS))
def test_every_coder(prod, both, orc, coder_table, name):
    img, offs, fbs = coder_table
    m = Moved(prod)
    g, t = check(prod, both, orc, CODERS[name], "i16", img, offs, fbs, what=name, out_phase=1)
    m.take()
    assert (m.launches, m.frames, m.batch) == (1, len(fbs), 0)
    assert (m.ck_launches, m.ck_frames) == (1, len(fbs))
    assert checksum_bits(g) == [1] * len(fbs)
    if name == "none-raw":
        assert g.sizes == [16 + fb + 4 for fb in fbs]  # the 16-byte header, the samples, the checksum
    else:
        assert all(len(f) >= 22 + 4 for f in frames_of(g))


# ---------------------------------------------------------------- 6. two passes
@pytest.mark.parametrize("secondary", ["none", "diff"])
def test_two_passes_share_one_checksum_launch(prod, both, orc, secondary):
    params = P(primary_preprocessing=eh.DIFF, primary_encoder_type=eh.GOLOMB_ZERO, primary_encoder_param=4,
               secondary_iterations=2, secondary_preprocessing=eh.NONE if secondary == "none" else eh.DIFF,
               secondary_encoder_type=eh.GOLOMB_MULTI, secondary_encoder_param=7, secondary_encoder_outlier=40,
               checksum_enabled=1)
    rng = np.random.default_rng(66)
    ns = [3000, 17, 16385, 4096, 33000, 1, 5000, 16384, 777]
    img, offs = eh.place([eh.stored(walk(rng, n, 3), True) for n in ns], MIXED)
    m = Moved(prod)
    g, t = check(prod, both, orc, params, "u16", img, offs, [2 * n for n in ns], big_endian=True)
    m.take()
    assert (m.launches, m.frames, m.batch) == (2, 9, 0)
    assert (m.ck_launches, m.ck_frames) == (1, 9)
    assert [f[14] for f in frames_of(g)] == [0, 1, 2] * 3  # header sequence numbers
    assert checksum_bits(g) == [1] * 9


# ---------------------------------------------------------------- 7. capacity cuts
def test_capacity_cuts_around_the_checksum_bytes(prod, both, orc):
    rng = np.random.default_rng(77)
    ns = [1000, 20000, 333, 16384, 500, 4097, 2, 1000]
    img, offs = eh.place([eh.stored(walk(rng, n), True) for n in ns], [2, 9])
    fbs = [2 * n for n in ns]
    params = P(**CK)
    t = eh.truth(orc, params, "u16", img, offs, fbs, big_endian=True)
    total = t.offsets[-1]
    end3 = t.offsets[4]  # the end of frame 3, its four checksum bytes included
    for capacity, fit in ((total, 8), (end3, 4), (end3 - 1, 3), (end3 - 2, 3), (end3 - 3, 3), (end3 - 4, 3),
                          (end3 - 5, 3), (total - 4, 7), (total - 1, 7)):
        m = Moved(prod)
        g = eh.run(prod, both, params, "u16", img, offs, fbs, big_endian=True, total=total, capacity=capacity,
                   out_phase=5)
        c = eh.cut(t, capacity)
        eh.same(g, c, capacity)  # the guards past out_offsets[num_frames] are part of it
        m.take()
        assert (m.launches, m.ck_launches) == (1, 1)
        assert g.sizes[:fit] == t.sizes[:fit] and eh.names(g.sizes[fit:]) == ["DST_TOO_SMALL"] * (8 - fit)
        assert t.image.startswith(g.image)


# ---------------------------------------------------------------- 8. several pieces
def test_a_small_chunk_cuts_the_table_into_pieces(prod, both, orc):
    rng = np.random.default_rng(88)
    ns = [2000 + 3 * i for i in range(12)] + [40000]
    img, offs = eh.place([eh.stored(walk(rng, n), True) for n in ns], MIXED)
    fbs = [2 * n for n in ns]
    params = P(**CK)
    t = eh.truth(orc, params, "u16", img, offs, fbs, big_endian=True)
    row = (fbs[0] + 15) // 16 * 16 + (prod.compress_bound(fbs[0]) + 7) // 8 * 8
    assert both.set_option(pkg.OPT_IMAGE_CHUNK, 5 * row + 200) == 0
    m = Moved(prod)
    g = eh.run(prod, both, params, "u16", img, offs, fbs, big_endian=True, total=t.offsets[-1])
    eh.same(g, t)
    m.take()
    assert m.launches >= 3 and m.ck_launches == m.launches  # one pass: a checksum launch per piece
    assert (m.frames, m.ck_frames, m.batch) == (len(ns), len(ns), 0)


def test_a_kept_run_between_two_ragged_pieces(prod, eng, orc):
    """Option 5 at 65536: eight equal 16 Ki-sample frames stay a RUN on the
    batch path (with its own checksum launches), the frames around them are
    two ragged pieces on the new path."""
    rng = np.random.default_rng(89)
    ns = [10, 11, 13, 3000] + [16384] * 8 + [7, 50, 50, 9, 1200]
    img, offs = eh.place([eh.stored(walk(rng, n), False) for n in ns], [0])
    fbs = [2 * n for n in ns]
    params = P(**CK)
    t = eh.truth(orc, params, "u16", img, offs, fbs)
    try:
        assert eng.set_option(pkg.OPT_IMAGE_RAGGED, 65536) == 0
        assert eng.set_option(pkg.OPT_IMAGE_RAGGED_CHECKSUM, 1) == 0
        m = Moved(prod)
        g = eh.run(prod, eng, params, "u16", img, offs, fbs, total=t.offsets[-1])
        eh.same(g, t)
        m.take()
        assert (m.launches, m.frames) == (2, len(ns) - 8)
        assert (m.ck_launches, m.ck_frames) == (2, len(ns) - 8)
        assert m.batch > 0 and m.emitted == len(ns)
        assert checksum_bits(g) == [1] * len(ns)
    finally:
        assert eng.set_option(pkg.OPT_IMAGE_RAGGED, 0) == 0
        assert eng.set_option(pkg.OPT_IMAGE_RAGGED_CHECKSUM, 0) == 0


# ---------------------------------------------------------------- 9. engine reuse
def test_two_calls_queued_back_to_back(prod, both, orc):
    """Different tables on one engine, one wait at the end: the second call's
    checksum tables and products follow the first's in stream order."""
    rng = np.random.default_rng(99)
    params = P(**CK)
    calls = []
    for ns, big_endian, start in (([5000, 16385, 3, 40000, 777, 12000], True, 7000),
                                  ([100, 33000, 16384, 9], False, 9000),
                                  ([70000, 1, 2, 3, 4, 5, 6, 7, 8000], True, 11000)):
        img, offs = eh.place([eh.stored(walk(rng, n), big_endian) for n in ns], MIXED)
        fbs = [2 * n for n in ns]
        t = eh.truth(orc, params, "u16", img, offs, fbs, big_endian=big_endian, ts_start=start)
        calls.append((t, dict(img=img, offs=offs, fbs=fbs, big_endian=big_endian, total=t.offsets[-1],
                              ts_start=start)))
    m = Moved(prod)
    queued = [eh.launch(prod, both, params, "u16", k["img"], k["offs"], k["fbs"], big_endian=k["big_endian"],
                        total=k["total"], ts_start=k["ts_start"]) for _, k in calls]
    for i, ((t, _), h) in enumerate(zip(calls, queued)):
        eh.same(eh.collect(both, h), t, i)
    m.take()
    assert (m.launches, m.ck_launches, m.ck_frames) == (3, 3, 6 + 4 + 9)


# ---------------------------------------------------------------- 10. the opt-in
def test_the_opt_in(prod, eng, orc):
    rng = np.random.default_rng(100)
    ns = [3000, 17, 4097, 1000, 16385, 5]
    img, offs = eh.place([eh.stored(walk(rng, n), True) for n in ns], [3, 8, 13])
    fbs = [2 * n for n in ns]
    t = eh.truth(orc, P(**CK), "u16", img, offs, fbs, big_endian=True)
    images = {}
    try:
        for opt5, opt6, want in ((1, 0, (0, 0)), (0, 1, (0, 0)), (1, 1, (1, 1))):
            assert eng.set_option(pkg.OPT_IMAGE_RAGGED, opt5) == 0
            assert eng.set_option(pkg.OPT_IMAGE_RAGGED_CHECKSUM, opt6) == 0
            m = Moved(prod)
            g = eh.run(prod, eng, P(**CK), "u16", img, offs, fbs, big_endian=True, total=t.offsets[-1])
            eh.same(g, t, (opt5, opt6))
            m.take()
            assert (m.launches, m.ck_launches) == want, (opt5, opt6)
            assert (m.batch > 0) == (want == (0, 0))
            images[opt5, opt6] = (g.sizes, g.offsets, g.image)
        assert images[1, 0] == images[1, 1] == images[0, 1]  # byte for byte
        # both on, no checksum in the context: ragged launches, no ragged checksum launch
        m = Moved(prod)
        g, _ = check(prod, eng, orc, P(**ZERO32), "u16", img, offs, fbs, big_endian=True)
        m.take()
        assert (m.launches, m.ck_launches, m.ck_frames, m.batch) == (1, 0, 0, 0)
        assert checksum_bits(g) == [0] * len(ns)
        assert eng.set_option(pkg.OPT_IMAGE_RAGGED_CHECKSUM, 2) == api.err_value("PARAMS_INVALID")
    finally:
        assert eng.set_option(pkg.OPT_IMAGE_RAGGED, 0) == 0
        assert eng.set_option(pkg.OPT_IMAGE_RAGGED_CHECKSUM, 0) == 0


# ---------------------------------------------------------------- 11. round trip
def test_round_trip_through_the_image_decoder(prod, both, orc):
    import torch
    rng = np.random.default_rng(111)
    S = segment(prod, "u16")
    ns = [1, 7, 8, 33, 1025, 4097, S, S + 1, 2 * S + 9, 100]
    img, offs = eh.place([eh.stored(walk(rng, n), True) for n in ns], MIXED)
    fbs = [2 * n for n in ns]
    g, t = check(prod, both, orc, P(**CK), "u16", img, offs, fbs, big_endian=True, out_phase=7)
    count, tab, bad = prod.frame_table(g.image)
    assert count == len(fbs) and bad is None and [int(o) for o in tab] == g.offsets[:-1]
    src = torch.from_numpy(np.frombuffer(g.image, dtype=np.uint8).copy()).cuda()
    dst = torch.zeros(sum(fbs) + 16, dtype=torch.uint8, device="cuda")
    st = torch.zeros(count, dtype=torch.int32, device="cuda")
    ck = torch.zeros(count, dtype=torch.uint8, device="cuda")
    rc, dof = both.decompress_image("u16", src.data_ptr(), len(g.image), tab, dst.data_ptr(), sum(fbs),
                                    st.data_ptr(), ck.data_ptr(), flags=pkg.IMG_BIG_ENDIAN)
    assert rc == 0 and both.synchronize() == 0
    assert [int(s) for s in st.cpu().numpy()] == ns
    assert [int(v) for v in ck.cpu().numpy()] == [1] * count
    out = dst.cpu().numpy()
    for f, (o, fb) in enumerate(zip(offs, fbs)):
        assert np.array_equal(out[int(dof[f]):int(dof[f + 1])], img[o:o + fb]), f


# ---------------------------------------------------------------- 12. CLI
def test_cli_directory_of_unequal_files_with_a_checksum(tmp_path, prod, orc):
    """airspace -c sets both options on its engine.  The output files against
    the oracle's loop, byte for byte but for the identifier (header bytes
    8-13), which the tool draws from the clock."""
    if not prod.gpu_available():
        pytest.fail("GPU test run without a usable HIP device")
    rng = np.random.default_rng(1212)
    ns = [1, 2, 777, 4096, 5000, 16384, 16385, 40000, 33, 9001]
    paths, xs = [], []
    for i, n in enumerate(ns):
        x = walk(rng, n)
        p = tmp_path / f"s{i:02d}.dat"
        p.write_bytes(x.astype(">u2").tobytes())
        paths.append(p)
        xs.append(x)
    arg = "primary_preprocessing=DIFF,primary_encoder_type=GOLOMB_ZERO,primary_encoder_param=32,checksum_enabled=1"
    r = subprocess.run([CLI, "-c", "--params", arg, "--quiet"] + [str(p) for p in paths], capture_output=True,
                       cwd=tmp_path, timeout=120)
    assert r.returncode == 0, r.stderr.decode()
    ctx = api.CmpContext()
    assert not api.is_error(orc.initialise(ctx, P(**CK)))
    for p, x in zip(paths, xs):
        cap = orc.compress_bound(2 * x.size)
        dst = api.aligned_empty(cap)
        size = orc.compress_u16(ctx, dst, cap, x)
        assert not api.is_error(size), api.error_name(size)
        got, want = (tmp_path / (p.name + ".air")).read_bytes(), bytes(dst[:size])
        assert want[15] & 8 and got[:8] + got[14:] == want[:8] + want[14:], p.name
