"""cmp_gpu_compress_image with CMP_GPU_OPT_IMAGE_RAGGED: frames of unequal sizes
in one ragged encode launch per pass (enc_ragged.hip).  The
option changes the schedule only, so truth is what it is without it: the CPU
oracle's call loop over the same table with the same timestamp function
(tests/encode_image_helpers.py).  After every call the sizes, the offsets, the
image bytes, the guards, the context's fields and the work buffer are compared;
the device layer's counters (airs_dev_ragged_stats, airs_dev_encode_image_stats,
airs_dev_launch_stats) say which way the frames went.

S below is the ragged kernel's segment in samples, asked of the library
(airs_dev_ragged_segment, which answers seg_chunks(W, 0) * 4096 of
enc_kernel.h): 16384 for 16-bit samples and 8192 for i16-in-i32 today."""
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
MIXED = [0, 5, 2, 11, 14, 7]  # byte phases of the frames in the sample image


@pytest.fixture(scope="module")
def eng(prod):
    """The ragged tests' own engine; every test sets the option it needs."""
    if not prod.gpu_available():
        pytest.fail("GPU test run without a usable HIP device")
    e = prod.engine()
    yield e
    e.close()


@pytest.fixture
def ragged(eng):
    assert eng.set_option(pkg.OPT_IMAGE_RAGGED, 1) == 0
    assert eng.set_option(pkg.OPT_IMAGE_CHUNK, 0) == 0
    yield eng
    assert eng.set_option(pkg.OPT_IMAGE_RAGGED, 0) == 0
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
        return (counters(self.prod, "airs_dev_ragged_stats", 3), eh.stage_frames(self.prod),
                counters(self.prod, "airs_dev_launch_stats", 10))

    def take(self):
        now = self.read()
        d = [[a - b for a, b in zip(n, o)] for n, o in zip(now, self.at)]
        self.at = now
        self.launches, self.frames, self.blocks = d[0]
        self.ingested, self.emitted, self.refused = d[1]
        self.batch = sum(d[2])
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


def frame_bytes(x, kind, big_endian):
    if kind == "i16_in_i32":
        return x.view(np.int16).astype(np.int32).view(np.uint8)
    return eh.stored(x, big_endian)


def edge_sizes(S, upto=None):
    sizes = [1, 2, 15, 16, 17, 4095, 4096, 4097, S - 1, S, S + 1, 2 * S, 2 * S + 5, 17 * S + 1, 65 * S + 9]
    return [n for n in sizes if upto is None or n <= upto]


def table(prod, kind, big_endian, phases, seed, upto=None):
    """The edge sizes in a shuffled order, each frame at the next position of
    the image whose byte phase is the next of `phases`."""
    rng = np.random.default_rng(seed)
    S = segment(prod, kind)
    ns = [int(n) for n in rng.permutation(edge_sizes(S, None if upto is None else upto(S)))]
    chunks = [frame_bytes(walk(rng, n), kind, big_endian) for n in ns]
    img, offs = eh.place(chunks, phases)
    return img, offs, [len(c) for c in chunks]


def check(prod, eng, orc, params, kind, img, offs, fbs, what="", primary_g=None, **kw):
    t = eh.truth(orc, params, kind, img, offs, fbs, big_endian=kw.get("big_endian", False), wbs=kw.get("wbs"),
                 primary_g=primary_g)
    g = eh.run(prod, eng, params, kind, img, offs, fbs, total=t.offsets[-1], **kw)
    eh.same(g, t, what)
    return g, t


def not_direct(kind, big_endian, offs, src_phase=0):
    """Frames a ragged piece stages: big-endian ones, and those whose address
    (the image starts at a 16-byte aligned address plus src_phase) is no
    multiple of the sample size."""
    return sum(1 for o in offs if big_endian or (o + src_phase) % eh.sample_bytes(kind))


# ---------------------------------------------------------------- 1. segment and chunk edges
EDGE_CASES = {
    "u16-be-mixed": ("u16", True, MIXED),
    "i16-native-aligned": ("i16", False, [0]),
    "i16-in-i32": ("i16_in_i32", False, [0, 4, 6, 12]),
}


@pytest.fixture(scope="module")
def edge_truth(prod, orc):
    """Table and truth of every edge case, computed once."""
    out = {}
    for name, (kind, big_endian, phases) in EDGE_CASES.items():
        img, offs, fbs = table(prod, kind, big_endian, phases, seed=101)
        out[name] = (img, offs, fbs, eh.truth(orc, P(**ZERO32), kind, img, offs, fbs, big_endian=big_endian))
    return out


@pytest.mark.parametrize("case", sorted(EDGE_CASES))
def test_segment_and_chunk_edges(prod, ragged, edge_truth, case):
    """17 S + 1 samples put a segment past the 16-granule scalar first window of
    the look-back, 65 S + 9 one past a whole 64-granule window."""
    kind, big_endian, _ = EDGE_CASES[case]
    img, offs, fbs, t = edge_truth[case]
    S = segment(prod, kind)
    assert S == (8192 if kind == "i16_in_i32" else 16384)
    assert max(fbs) == (65 * S + 9) * eh.sample_bytes(kind) and len(set(fbs)) == len(fbs) == 15
    m = Moved(prod)
    g = eh.run(prod, ragged, P(**ZERO32), kind, img, offs, fbs, big_endian=big_endian, total=t.offsets[-1],
               out_phase=3)
    eh.same(g, t, case)
    m.take()
    assert (m.launches, m.frames) == (1, len(fbs))
    assert m.blocks == sum(-(-fb // (S * eh.sample_bytes(kind))) for fb in fbs)
    assert (m.ingested, m.emitted, m.refused) == (not_direct(kind, big_endian, offs), len(fbs), 0)
    assert m.batch == 0
    if case == "i16-in-i32":
        assert 0 < m.ingested < len(fbs)


# ---------------------------------------------------------------- 2. coders
def coder(pre, enc, g=0, outlier=0):
    return P(primary_preprocessing=pre, primary_encoder_type=enc, primary_encoder_param=g,
             primary_encoder_outlier=outlier)


CODERS = {"none-raw": coder(eh.NONE, eh.UNCOMPRESSED)}
for _pre, _pn in ((eh.NONE, "none"), (eh.DIFF, "diff")):
    for _g in (1, 3, 1055, 4096, 32768):
        CODERS[f"{_pn}-zero{_g}"] = coder(_pre, eh.GOLOMB_ZERO, _g)
    for _g in (7, 16):
        CODERS[f"{_pn}-multi{_g}"] = coder(_pre, eh.GOLOMB_MULTI, _g, 40)


@pytest.fixture(scope="module")
def coder_table(prod):
    return table(prod, "i16", False, [0, 3, 2, 16 - 2, 9], seed=202, upto=lambda S: 2 * S + 5)


@pytest.mark.parametrize("name", sorted(CODERS))
def test_coders(prod, ragged, orc, coder_table, name):
    img, offs, fbs = coder_table
    assert len(fbs) == 13
    m = Moved(prod)
    g, t = check(prod, ragged, orc, CODERS[name], "i16", img, offs, fbs, what=name, out_phase=1)
    m.take()
    assert (m.launches, m.frames, m.batch) == (1, len(fbs), 0)
    assert m.ingested == not_direct("i16", False, offs)
    if name == "none-raw":
        assert t.sizes == [16 + fb for fb in fbs]  # 16-byte headers
    else:
        assert all(f[:2] == t.frames[0][:2] and len(f) >= 22 for f in t.frames)


# ---------------------------------------------------------------- 3. two passes
def test_two_passes_take_two_launches(prod, ragged, orc):
    params = P(primary_preprocessing=eh.DIFF, primary_encoder_type=eh.GOLOMB_ZERO, primary_encoder_param=4,
               secondary_iterations=2, secondary_preprocessing=eh.DIFF, secondary_encoder_type=eh.GOLOMB_MULTI,
               secondary_encoder_param=7, secondary_encoder_outlier=40)
    rng = np.random.default_rng(303)
    ns = [3000, 17, 16385, 4096, 33000, 1, 5000, 16384, 777]
    img, offs = eh.place([eh.stored(walk(rng, n, 3), True) for n in ns], MIXED)
    m = Moved(prod)
    g, t = check(prod, ragged, orc, params, "u16", img, offs, [2 * n for n in ns], big_endian=True)
    m.take()
    assert (m.launches, m.frames, m.batch) == (2, 9, 0)
    assert [f[14] for f in t.frames] == [0, 1, 2] * 3  # header sequence numbers
    ids = [f[8:14] for f in t.frames]  # one identifier per reset, carried by its secondary passes
    assert ids[0] == ids[1] == ids[2] != ids[3] == ids[4] == ids[5] != ids[6] == ids[7] == ids[8]
    got = [g.image[o:o + s] for o, s in zip(g.offsets, g.sizes)]
    assert [f[8:15] for f in got] == [f[8:15] for f in t.frames]


# ---------------------------------------------------------------- 4. direct and staged in one piece
def test_direct_and_staged_frames_share_a_piece(prod, ragged, orc):
    """Native u16: frames at odd addresses are staged, frames at 2-byte aligned
    addresses with irregular steps are read where they lie and add nothing to
    the ingest counter."""
    rng = np.random.default_rng(404)
    ns = [1000, 1001, 5000, 16385, 37, 1002, 20000, 999]
    phases = [0, 1, 6, 3, 10, 14, 5, 2]
    img, offs = eh.place([eh.stored(walk(rng, n), False) for n in ns], phases)
    odd = sum(o % 2 for o in offs)
    assert odd == 3 and len({b - a for a, b in zip(offs, offs[1:])}) == len(ns) - 1
    m = Moved(prod)
    check(prod, ragged, orc, P(**ZERO32), "u16", img, offs, [2 * n for n in ns])
    m.take()
    assert (m.launches, m.frames, m.ingested, m.emitted) == (1, len(ns), odd, len(ns))
    # the same table from an odd address: the other frames are the staged ones
    check(prod, ragged, orc, P(**ZERO32), "u16", img, offs, [2 * n for n in ns], src_phase=1)
    m.take()
    assert (m.launches, m.ingested) == (1, len(ns) - odd)


# ---------------------------------------------------------------- 5. refused frames inside the table
def test_refused_frames_split_the_pieces(prod, ragged, orc):
    params = P(primary_preprocessing=eh.DIFF, primary_encoder_type=eh.GOLOMB_ZERO, primary_encoder_param=7,
               secondary_iterations=2, secondary_preprocessing=eh.DIFF, secondary_encoder_type=eh.GOLOMB_ZERO,
               secondary_encoder_param=9)
    rng = np.random.default_rng(505)
    pool = frame_bytes(walk(rng, 6000), "i16_in_i32", False)
    offs, fbs = [0, 400, 8, 1000, 4000, 12, 9000, 9600], [64, 256, 0, 1024, 2000, 6, 400, 4 * 2049]
    m = Moved(prod)
    g, t = check(prod, ragged, orc, params, "i16_in_i32", pool, offs, fbs)
    m.take()
    assert eh.names(t.sizes)[2] == eh.names(t.sizes)[5] == "SRC_SIZE_WRONG"
    assert [f[14] for f in t.frames if f] == [0, 1, 2, 0, 1, 2]
    # pieces of 2 frames each: sequence numbers (0, 1), (2, 0) and (1, 2), so the
    # first two hold both passes and the last the secondary alone
    assert (m.frames, m.refused, m.emitted, m.batch) == (6, 2, 6, 0)
    assert m.launches == 2 + 2 + 1


# ---------------------------------------------------------------- 6. capacity
def test_capacity_ends_inside_a_piece(prod, ragged, orc):
    rng = np.random.default_rng(606)
    ns = [1000, 20000, 333, 16384, 500, 4097, 2, 1000]
    img, offs = eh.place([eh.stored(walk(rng, n), True) for n in ns], [2, 9])
    fbs = [2 * n for n in ns]
    params = P(**ZERO32)
    t = eh.truth(orc, params, "u16", img, offs, fbs, big_endian=True)
    total = t.offsets[-1]
    for capacity in (total, total - 1, t.offsets[3] + t.sizes[3] // 2, t.offsets[4], t.offsets[1], 0):
        m = Moved(prod)
        g = eh.run(prod, ragged, params, "u16", img, offs, fbs, big_endian=True, total=total, capacity=capacity,
                   out_phase=5)
        eh.same(g, eh.cut(t, capacity), capacity)
        assert m.take().launches == 1
    c = eh.cut(t, t.offsets[4])  # exactly at a frame's end
    assert c.sizes[:4] == t.sizes[:4] and eh.names(c.sizes[4:]) == ["DST_TOO_SMALL"] * 4


# ---------------------------------------------------------------- 7. budgets
def test_budgets_cut_pieces_not_bytes(prod, ragged, orc):
    rng = np.random.default_rng(707)
    ns = [2000 + 3 * i for i in range(12)] + [40000]
    img, offs = eh.place([eh.stored(walk(rng, n), True) for n in ns], MIXED)
    fbs = [2 * n for n in ns]
    params = P(**ZERO32)
    t = eh.truth(orc, params, "u16", img, offs, fbs, big_endian=True)
    row = (fbs[0] + 15) // 16 * 16 + (prod.compress_bound(fbs[0]) + 7) // 8 * 8
    launches = []
    for budget in (0, 5 * row + 200, row // 2):
        assert ragged.set_option(pkg.OPT_IMAGE_CHUNK, budget) == 0
        m = Moved(prod)
        g = eh.run(prod, ragged, params, "u16", img, offs, fbs, big_endian=True, total=t.offsets[-1])
        eh.same(g, t, budget)
        m.take()
        assert (m.frames, m.batch) == (len(ns), 0)
        launches.append(m.launches)
    assert launches[0] == 1 and launches[1] in (3, 4) and launches[2] == len(ns)


# ---------------------------------------------------------------- 8. the keep rule
def test_keep_rule(prod, eng, orc):
    """Option value 65536: a run of eight equal 16 Ki-sample frames (256 KiB of
    samples) stays on the batch path, a run of two equal 100-byte frames joins
    the ragged piece around it.  Value 1 (1 MiB) sends everything to ragged
    pieces, value 0 nothing; the bytes are the same."""
    rng = np.random.default_rng(808)
    ns = [10, 11, 13] + [16384] * 8 + [7, 50, 50, 9, 12]
    img, offs = eh.place([eh.stored(walk(rng, n), False) for n in ns], [0])
    fbs = [2 * n for n in ns]
    params = P(**ZERO32)
    t = eh.truth(orc, params, "u16", img, offs, fbs)
    try:
        for value, want in ((65536, (2, len(ns) - 8, True)), (1, (1, len(ns), False)), (0, (0, 0, True))):
            assert eng.set_option(pkg.OPT_IMAGE_RAGGED, value) == 0
            m = Moved(prod)
            g = eh.run(prod, eng, params, "u16", img, offs, fbs, total=t.offsets[-1])
            eh.same(g, t, value)
            m.take()
            assert (m.launches, m.frames, m.batch > 0) == want, value
            assert m.emitted == len(ns)
    finally:
        assert eng.set_option(pkg.OPT_IMAGE_RAGGED, 0) == 0


# ---------------------------------------------------------------- 9. ineligible contexts
MODEL3 = dict(primary_preprocessing=eh.DIFF, primary_encoder_type=eh.GOLOMB_ZERO, primary_encoder_param=16,
              secondary_iterations=3, secondary_preprocessing=eh.MODEL, secondary_encoder_type=eh.GOLOMB_MULTI,
              secondary_encoder_param=8, secondary_encoder_outlier=107, model_rate=11)
INELIGIBLE = {
    "model": (P(**MODEL3), 0),
    "iwt": (P(primary_preprocessing=eh.IWT, primary_encoder_type=eh.GOLOMB_ZERO, primary_encoder_param=4), 0),
    "checksum": (P(checksum_enabled=1, **ZERO32), 0),
    "fallback": (P(uncompressed_fallback_enabled=1, **ZERO32), 0),
    "auto-rice": (P(primary_preprocessing=eh.DIFF, primary_encoder_type=eh.GOLOMB_ZERO, primary_encoder_param=3),
                  api.GPU_AUTO_RICE),
}


@pytest.mark.parametrize("what", sorted(INELIGIBLE))
def test_ineligible_contexts_take_the_runs(prod, ragged, orc, orc_ext, what):
    params, flags = INELIGIBLE[what]
    rng = np.random.default_rng(909)
    ns = [3000] * 4 + [1000] + [3000] * 2 + [17, 4097]  # MODEL: the size change is a per-frame error
    img, offs = eh.place([eh.stored(walk(rng, n, 3), True) for n in ns], [3, 8, 13])
    m = Moved(prod)
    g, t = check(prod, ragged, orc, params, "u16", img, offs, [2 * n for n in ns], big_endian=True,
                 batch_flags=flags, primary_g=eh.select_g(orc_ext, "u16", eh.DIFF) if flags else None, what=what)
    m.take()
    assert (m.launches, m.frames, m.blocks) == (0, 0, 0)
    assert m.batch > 0
    if what == "model":
        assert "SRC_SIZE_MISMATCH" in eh.names(t.sizes)


# ---------------------------------------------------------------- 10. engine reuse
def test_two_calls_queued_back_to_back(prod, ragged, orc):
    """Different tables and piece sizes on one engine, one wait at the end: the
    second call's tables and rows follow the first's in stream order."""
    rng = np.random.default_rng(1010)
    params = P(**ZERO32)
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
    queued = [eh.launch(prod, ragged, params, "u16", k["img"], k["offs"], k["fbs"], big_endian=k["big_endian"],
                        total=k["total"], ts_start=k["ts_start"]) for _, k in calls]
    for i, ((t, _), h) in enumerate(zip(calls, queued)):
        eh.same(eh.collect(ragged, h), t, i)
    assert m.take().launches == 3


# ---------------------------------------------------------------- 11. round trip
def test_round_trip_through_the_image_decoder(prod, ragged, edge_truth):
    import torch
    img, offs, fbs, t = edge_truth["u16-be-mixed"]
    g = eh.run(prod, ragged, P(**ZERO32), "u16", img, offs, fbs, big_endian=True, total=t.offsets[-1], out_phase=7)
    eh.same(g, t)
    count, tab, bad = prod.frame_table(g.image)
    assert count == len(fbs) and bad is None and [int(o) for o in tab] == g.offsets[:-1]
    src = torch.from_numpy(np.frombuffer(g.image, dtype=np.uint8).copy()).cuda()
    dst = torch.zeros(sum(fbs) + 16, dtype=torch.uint8, device="cuda")
    st = torch.zeros(count, dtype=torch.int32, device="cuda")
    ck = torch.zeros(count, dtype=torch.uint8, device="cuda")
    rc, dof = ragged.decompress_image("u16", src.data_ptr(), len(g.image), tab, dst.data_ptr(), sum(fbs),
                                      st.data_ptr(), ck.data_ptr(), flags=pkg.IMG_BIG_ENDIAN)
    assert rc == 0 and ragged.synchronize() == 0
    assert [int(s) for s in st.cpu().numpy()] == [fb // 2 for fb in fbs]
    out = dst.cpu().numpy()
    for f, (o, fb) in enumerate(zip(offs, fbs)):
        assert np.array_equal(out[int(dof[f]):int(dof[f + 1])], img[o:o + fb]), f


# ---------------------------------------------------------------- 12. CLI
def test_cli_directory_of_all_different_sizes(tmp_path, prod, orc):
    """airspace -c sets the option on its engine: a directory of files that all
    differ in size is one ragged piece.  The output files against the oracle's
    loop, byte for byte but for the identifier (header bytes 8-13), which the
    tool draws from the clock."""
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
    par = dict(primary_preprocessing=eh.DIFF, primary_encoder_type=eh.GOLOMB_ZERO, primary_encoder_param=32,
               secondary_iterations=2, secondary_preprocessing=eh.DIFF, secondary_encoder_type=eh.GOLOMB_MULTI,
               secondary_encoder_param=7, secondary_encoder_outlier=40)
    names = {"primary_preprocessing": ["NONE", "DIFF"], "secondary_preprocessing": ["NONE", "DIFF"],
             "primary_encoder_type": ["UNCOMPRESSED", "GOLOMB_ZERO", "GOLOMB_MULTI"],
             "secondary_encoder_type": ["UNCOMPRESSED", "GOLOMB_ZERO", "GOLOMB_MULTI"]}
    arg = ",".join(f"{k}={names[k][v] if k in names else v}" for k, v in par.items())
    r = subprocess.run([CLI, "-c", "--params", arg, "--quiet"] + [str(p) for p in paths], capture_output=True,
                       cwd=tmp_path, timeout=120)
    assert r.returncode == 0, r.stderr.decode()
    ctx = api.CmpContext()
    assert not api.is_error(orc.initialise(ctx, P(**par)))
    for p, x in zip(paths, xs):
        cap = orc.compress_bound(2 * x.size)
        dst = api.aligned_empty(cap)
        size = orc.compress_u16(ctx, dst, cap, x)
        assert not api.is_error(size), api.error_name(size)
        got, want = (tmp_path / (p.name + ".air")).read_bytes(), bytes(dst[:size])
        assert got[:8] + got[14:] == want[:8] + want[14:], p.name
