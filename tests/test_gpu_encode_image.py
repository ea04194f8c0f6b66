"""cmp_gpu_compress_image: sample frames as they are stored -- at any byte
phase of one device buffer, of unequal sizes, big-endian or native -- compressed
as one context into a packed .air image with its offset table.  Truth is the
CPU oracle's call loop over the same table with the same timestamp function
(tests/encode_image_helpers.py); after every call the sizes, the offsets, the
image bytes, the 0xAB guard around the image, the context's fields and the work
buffer are compared."""
import numpy as np
import pytest

import encode_image_helpers as eh
from conftest import load_pkg

pytestmark = pytest.mark.gpu
pkg = load_pkg()
api = pkg.cmpapi
P = api.CmpParams

TILE = 16384  # encode_image.hip: the emit kernel's tile (IMG_TILE)
COUNTS = (1, 2, 7, 8, 9, 63, 64, 65, 4095, 4096, 4097)
RAW = dict(primary_preprocessing=eh.NONE, primary_encoder_type=eh.UNCOMPRESSED)


@pytest.fixture(scope="module")
def eng(prod):
    if not prod.gpu_available():
        pytest.fail("GPU test run without a usable HIP device")
    e = prod.engine()
    yield e
    e.close()


def check(prod, eng, orc, params, kind, img, offs, fbs, what="", primary_g=None, **kw):
    t = eh.truth(orc, params, kind, img, offs, fbs, big_endian=kw.get("big_endian", False), wbs=kw.get("wbs"),
                 primary_g=primary_g)
    g = eh.run(prod, eng, params, kind, img, offs, fbs, total=t.offsets[-1], **kw)
    eh.same(g, t, what)
    return g, t


# ---------------------------------------------------------------- phases and edges
def edge_table(kind):
    """Every count twice, in a shuffled order, over a pool of random bytes: the
    source offsets walk all 16 byte phases, go back and forth and overlap."""
    rng = np.random.default_rng(18)  # an order in which the destinations reach every phase too
    sb = eh.sample_bytes(kind)
    pool = rng.integers(0, 256, 4 * 4097 * sb + 64, dtype=np.uint8)
    counts = list(COUNTS) + list(COUNTS)
    order = rng.permutation(len(counts))
    offs, fbs = [], []
    for i, j in enumerate(order):
        fb = counts[j] * sb
        base = int(rng.integers(0, (pool.size - fb - 16) // 16)) * 16
        offs.append(base + (5 * i + 3) % 16)
        fbs.append(fb)
    assert {o % 16 for o in offs} == set(range(16))
    assert any(offs[i + 1] < offs[i] for i in range(len(offs) - 1))
    assert any(a < b < a + fa for a, fa in zip(offs, fbs) for b in offs)
    return pool, offs, fbs


@pytest.mark.parametrize("out_phase", [0, 1])
@pytest.mark.parametrize("kind,big_endian", [("u16", True), ("u16", False), ("i16", True), ("i16", False),
                                             ("i16_in_i32", False)])
def test_every_phase_and_edge_count(prod, eng, orc, kind, big_endian, out_phase):
    """NONE + UNCOMPRESSED: a frame is 16 + 2n bytes, so the destination offsets
    walk the phases too (the even ones from an even out, the odd ones from an
    odd out)."""
    pool, offs, fbs = edge_table(kind)
    g, t = check(prod, eng, orc, P(**RAW), kind, pool, offs, fbs, big_endian=big_endian, out_phase=out_phase,
                 src_phase=out_phase * 7)
    assert t.sizes == [16 + 2 * (fb // eh.sample_bytes(kind)) for fb in fbs]
    assert {(g.out_ptr + o) % 16 for o in g.offsets[:-1]} == set(range(out_phase, 16, 2))


# ---------------------------------------------------------------- emit tile edges
SPANS = (TILE - 1, TILE, TILE + 1, 2 * TILE + 5)


def tile_table(out_phase, checksum):
    """UNCOMPRESSED frames, each after a one-sample neighbour that moves the
    destination phase on by 18 (or 22) bytes.  A frame's size is even, so the
    count of bytes that follow its head (size - head: what the emit kernel cuts
    into lines and tiles) takes the odd values of SPANS from an odd out and the
    even one from an even out; the spans that out_phase's parity allows are
    built, each with the head the destination phase gives it."""
    rng = np.random.default_rng(23)
    extra = 16 + (4 if checksum else 0)
    chunks, spans, pos = [], [], out_phase
    for want in SPANS:
        head = -(pos + 2 + extra) % 16  # after the neighbour
        size = want + head
        if size % 2:
            continue
        n = (size - extra) // 2
        chunks += [eh.stored(rng.integers(0, 65536, 1).astype(np.uint16), True),
                   eh.stored(rng.integers(0, 65536, n).astype(np.uint16), True)]
        spans.append(want)
        pos += 2 + extra + size
    img, offs = eh.place(chunks, [1, 2])
    return img, offs, [len(c) for c in chunks], spans


@pytest.mark.parametrize("checksum", [0, 1])
def test_emit_tile_edges(prod, eng, orc, checksum):
    seen = []
    for out_phase in (0, 1):
        img, offs, fbs, spans = tile_table(out_phase, checksum)
        g, t = check(prod, eng, orc, P(checksum_enabled=checksum, **RAW), "u16", img, offs, fbs, big_endian=True,
                     out_phase=out_phase, what=out_phase)
        for f in range(1, len(fbs), 2):  # the bytes after the head, as the emit kernel cuts them
            seen.append(g.sizes[f] - (-(g.out_ptr + g.offsets[f]) % 16))
        assert seen[-len(spans):] == spans
    assert sorted(seen) == sorted(SPANS)


# ---------------------------------------------------------------- coders
def run_table(rng, big_endian, singles=(77, 4097)):
    """Three runs (5 x 1000, 1 x 333, 4 x 1000 samples) and singletons, smooth
    samples, at odd and even phases of the image."""
    ns = [1000] * 5 + [333] + [1000] * 4 + list(singles)
    chunks = [eh.stored(eh.smooth(rng, n), big_endian) for n in ns]
    img, offs = eh.place(chunks, [0, 5, 2, 11, 16 - 2, 7])
    return img, offs, [2 * n for n in ns]


CODERS = {
    "diff-zero32": (P(primary_preprocessing=eh.DIFF, primary_encoder_type=eh.GOLOMB_ZERO, primary_encoder_param=32,
                      checksum_enabled=1), 0),
    "diff-multi11": (P(primary_preprocessing=eh.DIFF, primary_encoder_type=eh.GOLOMB_MULTI, primary_encoder_param=11,
                       primary_encoder_outlier=40), 0),
    "iwt-zero4": (P(primary_preprocessing=eh.IWT, primary_encoder_type=eh.GOLOMB_ZERO, primary_encoder_param=4,
                    checksum_enabled=1), 0),
    "auto-rice": (P(primary_preprocessing=eh.DIFF, primary_encoder_type=eh.GOLOMB_ZERO, primary_encoder_param=3), 1),
}


@pytest.mark.parametrize("big_endian", [True, False], ids=["be", "native"])
@pytest.mark.parametrize("coder", sorted(CODERS))
def test_coders_over_runs_and_singletons(prod, eng, orc, orc_ext, coder, big_endian):
    params, flags = CODERS[coder]
    img, offs, fbs = run_table(np.random.default_rng(31), big_endian)
    g, t = check(prod, eng, orc, params, "u16", img, offs, fbs, big_endian=big_endian, batch_flags=flags,
                 primary_g=eh.select_g(orc_ext, "u16", eh.DIFF) if flags else None)
    assert not any(api.is_error(s) for s in t.sizes)
    assert sum(t.sizes) < sum(fbs) // 2, "the samples do not compress: the table tests nothing"


# ---------------------------------------------------------------- MODEL
MODEL3 = dict(primary_preprocessing=eh.DIFF, primary_encoder_type=eh.GOLOMB_ZERO, primary_encoder_param=16,
              secondary_iterations=3, secondary_preprocessing=eh.MODEL, secondary_encoder_type=eh.GOLOMB_MULTI,
              secondary_encoder_param=8, secondary_encoder_outlier=107, model_rate=11, checksum_enabled=1)


def acquisitions(rng, n, count, noisy=()):
    base = 30000 + np.cumsum(rng.integers(-3, 4, n))
    return [((rng.integers(0, 65536, n) if a in noisy else base + rng.integers(-4, 5, n)) & 0xFFFF).astype(np.uint16)
            for a in range(count)]


@pytest.mark.parametrize("n", [4096, 3001])
def test_model_context_with_a_size_change(prod, eng, orc, n):
    """Six equal frames (a primary pass, three secondary ones, the reset's
    primary pass, a secondary one), a frame of another size, three more of the
    first size: the odd frame is CMP_ERR_SRC_SIZE_MISMATCH and takes no bytes."""
    rng = np.random.default_rng(n)
    xs = acquisitions(rng, n, 6) + [eh.smooth(rng, 1000)] + acquisitions(rng, n, 3)
    img, offs = eh.place([eh.stored(x, True) for x in xs], [3, 8, 13])
    g, t = check(prod, eng, orc, P(**MODEL3), "u16", img, offs, [2 * x.size for x in xs], big_endian=True)
    assert api.error_name(t.sizes[6]) == "SRC_SIZE_MISMATCH" and t.offsets[6] == t.offsets[7]
    assert [api.is_error(s) for s in t.sizes] == [False] * 6 + [True] + [False] * 3
    assert [f[14] for f in t.frames if f] == [0, 1, 2, 3, 0, 1, 2, 3, 0]  # the passes, by sequence number


@pytest.mark.parametrize("batch_flags", [0, api.GPU_HOST_STEPPED], ids=["device", "host-stepped"])
def test_model_context_with_the_uncompressed_fallback(prod, eng, orc, batch_flags):
    """Two noisy frames fall back: the synchronising path, three and two draws."""
    rng = np.random.default_rng(77)
    n = 4096
    xs = acquisitions(rng, n, 8, noisy=(2, 5))
    img, offs = eh.place([eh.stored(x, False) for x in xs], [0])
    params = P(uncompressed_fallback_enabled=1, **MODEL3)
    g, t = check(prod, eng, orc, params, "u16", img, offs, [2 * n] * 8, batch_flags=batch_flags)
    raw = [f for f in t.frames if api.parse_header(f)["encoder_type"] == eh.UNCOMPRESSED]
    # the noisy frames, and the frames coded against the model a noisy frame left
    assert 2 <= len(raw) < 8 and all(len(f) == 16 + 2 * n + 4 for f in raw)


# ---------------------------------------------------------------- per-frame errors
def test_frames_the_loop_refuses(prod, eng, orc):
    """A zero and an odd frame_bytes, and (i16-in-i32) one that is no multiple
    of four, get the loop's value, take no bytes and leave the context alone."""
    rng = np.random.default_rng(5)
    pool = rng.integers(0, 256, 4096, dtype=np.uint8)
    params = P(primary_preprocessing=eh.DIFF, primary_encoder_type=eh.GOLOMB_ZERO, primary_encoder_param=7,
               secondary_iterations=2, secondary_preprocessing=eh.DIFF, secondary_encoder_type=eh.GOLOMB_ZERO,
               secondary_encoder_param=9)
    offs, fbs = [0, 100, 7, 7, 300, 4096, 9], [64, 0, 3, 3, 64, 0, 64]
    g, t = check(prod, eng, orc, params, "u16", pool, offs, fbs)
    assert eh.names(t.sizes)[1:4] == ["SRC_SIZE_WRONG"] * 3 and eh.names(t.sizes)[5] == "SRC_SIZE_WRONG"
    g, t = check(prod, eng, orc, params, "i16_in_i32", pool, [4, 8, 101], [64, 6, 64])
    assert eh.names(t.sizes)[1] == "SRC_SIZE_WRONG"
    # a table of refused frames only: the first launch is the scan's alone
    g, t = check(prod, eng, orc, params, "u16", pool, [1, 2], [0, 5])
    assert g.offsets == [0, 0, 0]


def test_work_buffer_too_small_for_some_frames(prod, eng, orc):
    rng = np.random.default_rng(6)
    xs = [eh.smooth(rng, n) for n in (500, 500, 500, 500, 800, 500)]  # frame 4 is a primary pass
    img, offs = eh.place([eh.stored(x, True) for x in xs], [1])
    g, t = check(prod, eng, orc, P(**MODEL3), "u16", img, offs, [2 * x.size for x in xs], big_endian=True, wbs=1000)
    assert eh.names(t.sizes)[4] == "WORK_BUF_TOO_SMALL" and not any(api.is_error(s) for s in t.sizes[:4])


# ---------------------------------------------------------------- direct and staged
def test_direct_and_staged_runs_agree(prod, eng, orc):
    """Equal frames at a constant stride.  Native samples whose first frame is
    2-byte aligned are read where they are, at a stride that is a multiple of
    16 and at one that is not (no frame goes through the ingest copy: the
    device layer's counters); the same bytes from an odd address and big-endian
    samples are staged (every frame does).  All give the same image."""
    rng = np.random.default_rng(41)
    n, nf = 2048, 8
    xs = [eh.smooth(rng, n) for _ in range(nf)]
    params = CODERS["diff-zero32"][0]
    images = []
    for stride, first, big_endian, src_phase, direct in ((2 * n + 32, 0, False, 0, True),
                                                         (2 * n + 32, 0, False, 2, True),
                                                         (2 * n + 6, 2, False, 0, True),
                                                         (2 * n + 6, 2, False, 14, True),
                                                         (2 * n, 0, False, 0, True),
                                                         (2 * n + 32, 0, False, 3, False),
                                                         (2 * n + 6, 1, False, 0, False),
                                                         (2 * n + 5, 0, False, 0, False),
                                                         (2 * n + 32, 0, True, 0, False),
                                                         (2 * n + 6, 2, True, 9, False)):
        offs = [first + f * stride for f in range(nf)]
        img = np.full(first + nf * stride, 0x33, dtype=np.uint8)
        for o, x in zip(offs, xs):
            img[o:o + 2 * n] = eh.stored(x, big_endian)
        before = eh.stage_frames(prod)
        g, t = check(prod, eng, orc, params, "u16", img, offs, [2 * n] * nf, big_endian=big_endian,
                     src_phase=src_phase, what=(stride, first, big_endian, src_phase))
        ingested, emitted, refused = (a - b for a, b in zip(eh.stage_frames(prod), before))
        assert (ingested, emitted, refused) == (0 if direct else nf, nf, 0), (stride, first, big_endian, src_phase)
        images.append((g.image, g.offsets, g.sizes))
    assert all(i == images[0] for i in images)


def test_direct_and_staged_runs_mix_in_one_table(prod, eng, orc):
    """Native samples: an aligned run at a constant stride (direct), a run whose
    offsets step unevenly (staged), an aligned singleton (direct), a refused
    frame, a run that goes backwards (staged)."""
    rng = np.random.default_rng(42)
    pool = eh.stored(eh.smooth(rng, 20000), False)
    offs = [0, 2100, 4200] + [8000, 10100, 12300] + [16000] + [5] + [30000, 27000]
    fbs = [2000] * 3 + [1800] * 3 + [1500] + [7] + [2000] * 2
    before = eh.stage_frames(prod)
    check(prod, eng, orc, CODERS["diff-zero32"][0], "u16", pool, offs, fbs)
    assert [a - b for a, b in zip(eh.stage_frames(prod), before)] == [3 + 2, 9, 1]


# ---------------------------------------------------------------- capacity
def test_capacity_cuts_a_prefix(prod, eng, orc):
    rng = np.random.default_rng(43)
    ns = [1000, 1000, 1000, 500, 500, 1000, 333, 1000]
    img, offs = eh.place([eh.stored(eh.smooth(rng, n), True) for n in ns], [2, 9])
    fbs = [2 * n for n in ns]
    params = CODERS["diff-zero32"][0]
    t = eh.truth(orc, params, "u16", img, offs, fbs, big_endian=True)
    total = t.offsets[-1]
    for capacity in (total, total - 1, t.offsets[3] + t.sizes[3] // 2, t.offsets[4], 0):
        g = eh.run(prod, eng, params, "u16", img, offs, fbs, big_endian=True, total=total, capacity=capacity,
                   out_phase=5)
        eh.same(g, eh.cut(t, capacity), capacity)
    # the cut in the middle of frame 3, spelled out
    c = eh.cut(t, t.offsets[3] + t.sizes[3] // 2)
    assert c.sizes[:3] == t.sizes[:3] and eh.names(c.sizes[3:]) == ["DST_TOO_SMALL"] * 5
    assert c.offsets[3:] == [t.offsets[3]] * 6 and c.image == t.image[:t.offsets[3]]
    assert eh.names(eh.cut(t, total - 1).sizes) == t.sizes[:7] + ["DST_TOO_SMALL"]


# ---------------------------------------------------------------- chunk budget
def test_chunk_budget_does_not_change_the_image(prod, orc):
    img, offs, fbs = run_table(np.random.default_rng(47), True)
    params = CODERS["diff-zero32"][0]
    t = eh.truth(orc, params, "u16", img, offs, fbs, big_endian=True)
    row = (2000 + 15) // 16 * 16 + (prod.compress_bound(2000) + 7) // 8 * 8
    e = prod.engine()
    try:
        for budget in (0, row, 3 * row):
            assert e.set_option(pkg.OPT_IMAGE_CHUNK, budget) == 0
            g = eh.run(prod, e, params, "u16", img, offs, fbs, big_endian=True, total=t.offsets[-1])
            eh.same(g, t, budget)
    finally:
        e.close()


# ---------------------------------------------------------------- round trip
def test_round_trip_through_the_image_decoder(prod, eng, orc):
    import torch
    img, offs, fbs = run_table(np.random.default_rng(53), True)
    params = CODERS["diff-zero32"][0]
    g, t = check(prod, eng, orc, params, "u16", img, offs, fbs, big_endian=True, out_phase=3)
    count, table, bad = prod.frame_table(g.image)
    assert count == len(fbs) and bad is None and [int(o) for o in table] == g.offsets[:-1]
    src = torch.from_numpy(np.frombuffer(g.image, dtype=np.uint8).copy()).cuda()
    dst = torch.zeros(sum(fbs) + 16, dtype=torch.uint8, device="cuda")
    st = torch.zeros(count, dtype=torch.int32, device="cuda")
    ck = torch.zeros(count, dtype=torch.uint8, device="cuda")
    rc, dof = eng.decompress_image("u16", src.data_ptr(), len(g.image), table, dst.data_ptr(), sum(fbs),
                                   st.data_ptr(), ck.data_ptr(), flags=pkg.IMG_BIG_ENDIAN)
    assert rc == 0 and eng.synchronize() == 0
    assert [int(s) for s in st.cpu().numpy()] == [fb // 2 for fb in fbs]
    assert [int(c) for c in ck.cpu().numpy()] == [1] * count
    out = dst.cpu().numpy()
    for f, (o, fb) in enumerate(zip(offs, fbs)):
        assert np.array_equal(out[int(dof[f]):int(dof[f + 1])], img[o:o + fb]), f


# ---------------------------------------------------------------- engine reuse
def test_engine_reuse_without_a_wait_between_calls(prod, eng, orc):
    """An image call, a cmp_gpu_compress batch right behind it (no wait in
    between; both use the engine's scratch), the image call again."""
    import torch
    img, offs, fbs = run_table(np.random.default_rng(59), True)
    params = P(**MODEL3)
    t = eh.truth(orc, params, "u16", img, offs, fbs, big_endian=True)
    h1 = eh.launch(prod, eng, params, "u16", img, offs, fbs, big_endian=True, total=t.offsets[-1])
    # the batch: 3 contexts of 4 frames
    n, nctx, fpc = 2048, 3, 4
    x = np.concatenate([eh.smooth(np.random.default_rng(c), n) for c in range(nctx * fpc)])
    src = torch.from_numpy(x.view(np.int16)).cuda()
    cap = prod.compress_bound(2 * n)
    dstride = (cap + 7) // 8 * 8
    dst = torch.zeros(nctx * fpc * dstride, dtype=torch.uint8, device="cuda")
    sizes = torch.zeros(nctx * fpc, dtype=torch.int32, device="cuda")
    ctxs = pkg.context_array(nctx)
    bp = CODERS["diff-zero32"][0]
    prod.set_timestamp_func(eh.ts_counter(100))
    try:
        for c in range(nctx):
            assert not api.is_error(prod.initialise(ctxs[c], bp))
        assert eng.compress(ctxs, fpc, "u16", src.data_ptr(), 2 * n, 2 * n, dst.data_ptr(), dstride, cap,
                            sizes.data_ptr()) == 0
    finally:
        prod.set_timestamp_func(None)
    g1 = eh.collect(eng, h1)
    eh.same(g1, t, "first")
    # the batch against the loop
    orc.set_timestamp_func(eh.ts_counter(100))
    try:
        host, sz = dst.cpu().numpy(), sizes.cpu().numpy()
        octx = [api.CmpContext() for _ in range(nctx)]
        for ctx in octx:
            assert not api.is_error(orc.initialise(ctx, bp))
        for c, ctx in enumerate(octx):
            for a in range(fpc):
                f = c * fpc + a
                ref = api.aligned_empty(cap)
                r = orc.compress_u16(ctx, ref, cap, x[f * n:(f + 1) * n])
                assert int(sz[f]) == r and bytes(host[f * dstride:f * dstride + r]) == bytes(ref[:r]), f
    finally:
        orc.set_timestamp_func(None)
    g3 = eh.run(prod, eng, params, "u16", img, offs, fbs, big_endian=True, total=t.offsets[-1])
    eh.same(g3, t, "again")
    assert (g3.image, g3.offsets, g3.sizes, g3.state, g3.work) == (g1.image, g1.offsets, g1.sizes, g1.state, g1.work)
