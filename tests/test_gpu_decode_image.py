"""cmp_gpu_decompress_image: frames as they are stored -- back to back at byte
granularity, at shuffled offsets, at the 8-byte aligned offsets of
cmp_gpu_pack_frames -- decoded from one device buffer and a host table into
samples packed back to back.  Truth is the encoder (the CPU oracle's call
loop); statuses, checksum_ok, model and model_n are also compared with a
strided one-context cmp_gpu_decompress_sequences call over the same frames."""
import numpy as np
import pytest

import image_helpers as ih
from conftest import load_pkg

pytestmark = pytest.mark.gpu
pkg = load_pkg()
api = pkg.cmpapi

SIZES = (1, 7, 8, 9, 2047, 2048, 2049, 4097)
KINDS = ("u16", "i16", "i16_in_i32")
NSEQ, N = 12, 3001  # tests/test_gpu_cli_seq.py's sequence


@pytest.fixture(scope="module")
def eng(prod):
    if not prod.gpu_available():
        pytest.fail("GPU test run without a usable HIP device")
    e = prod.engine()
    yield e
    e.close()


@pytest.fixture(scope="module")
def mixed(orc):
    """24 independent frames: every size in each sample type, NONE / DIFF / IWT
    cycling, GOLOMB_ZERO with one UNCOMPRESSED and GOLOMB_MULTI frames."""
    rng = np.random.default_rng(101)
    frames, xs = [], []
    for i, (kind, n) in enumerate((k, n) for k in KINDS for n in SIZES):
        enc = ih.GOLOMB_MULTI if i % 5 == 2 else ih.UNCOMPRESSED if i == 13 else ih.GOLOMB_ZERO
        prm = api.CmpParams(primary_preprocessing=i % 3, primary_encoder_type=enc, primary_encoder_param=5 + i,
                            primary_encoder_outlier=40, checksum_enabled=i % 2)
        f, x, _ = ih.oracle_sequence(orc, prm, kind, n, rng, 1)
        frames += f
        xs += x
    return frames, xs


def check_samples(r, xs, big_endian=False, which=None):
    for f, x in enumerate(xs):
        if which is not None and f not in which:
            continue
        assert r.status[f] == len(x), (f, ih.name(r.status[f]))
        assert np.array_equal(ih.frame_samples(r, f, big_endian), x), f


def test_mixed_sizes_every_phase(eng, mixed):
    frames, xs = mixed
    assert {f[15] >> 4 for f in frames} == {0, 1, 2} and {f[15] & 7 for f in frames} == {0, 1, 2}
    offs, size = ih.back_to_back(frames)
    assert len({o % 16 for o in offs}) >= 8, sorted({o % 16 for o in offs})
    img = ih.place(frames, offs, size, 0)
    first = None
    for phase in range(16):
        r = ih.run_image(eng, "u16", img, offs, phase=phase)
        assert r.rc == 0, (phase, ih.name(r.rc))
        assert r.dof == [int(v) for v in np.concatenate([[0], np.cumsum([2 * len(x) for x in xs])])]
        check_samples(r, xs)
        assert ih.guards_intact(r), phase
        if first is None:
            first = r
            ih.same_as_strided(eng, "u16", frames, r, max(SIZES))
        else:
            assert r.status == first.status and r.ck == first.ck and r.model_n == first.model_n, phase
            assert np.array_equal(r.out, first.out) and np.array_equal(r.model, first.model), phase


def test_big_endian_heads_and_tails(eng, mixed):
    """The frames' destinations start at every even phase of a 16-byte line
    (sizes 1, 7, 9 ... shift them): the swapped form through the same heads,
    lines and tails."""
    frames, xs = mixed
    offs, size = ih.back_to_back(frames)
    r = ih.run_image(eng, "u16", ih.place(frames, offs, size, 0), offs, flags=pkg.IMG_BIG_ENDIAN)
    assert r.rc == 0
    assert len({d % 16 for d in r.dof[:-1]}) >= 4
    check_samples(r, xs, big_endian=True)
    assert ih.guards_intact(r)


@pytest.fixture(scope="module", params=["u16", "i16"])
def sequence(request, orc):
    """12 frames of 3001 samples: DIFF primaries, MODEL secondaries with a
    reset inside, checksums, and one noisy acquisition that falls back to a raw
    frame in mid-sequence."""
    rng = np.random.default_rng(12)
    prm = api.CmpParams(primary_preprocessing=ih.DIFF, primary_encoder_type=ih.GOLOMB_ZERO, primary_encoder_param=16,
                        secondary_iterations=4, secondary_preprocessing=ih.MODEL,
                        secondary_encoder_type=ih.GOLOMB_MULTI, secondary_encoder_param=8,
                        secondary_encoder_outlier=107, model_rate=11, checksum_enabled=1,
                        uncompressed_fallback_enabled=1)
    frames, xs, model = ih.oracle_sequence(orc, prm, request.param, N, rng, NSEQ, noisy=(7,), step=20)
    pres = [f[15] >> 4 for f in frames]
    assert pres[:7] == [1, 3, 3, 3, 3, 1, 3], pres  # MODEL frames, a reset inside
    raw_mid = [i for i, f in enumerate(frames) if i and f[15] & 0xF7 == 0 and f[14] == 0]
    assert 7 in raw_mid, "no raw fallback frame in mid-sequence"
    assert any(pres[i + 1] == 3 for i in raw_mid if i + 1 < NSEQ), "no MODEL frame after a fallback"
    return request.param, frames, xs, model


@pytest.mark.parametrize("big_endian", [False, True])
def test_model_sequence(eng, sequence, big_endian):
    kind, frames, xs, model = sequence
    offs, size = ih.back_to_back(frames)
    r = ih.run_image(eng, kind, ih.place(frames, offs, size, 0), offs, phase=5,
                     flags=pkg.IMG_BIG_ENDIAN if big_endian else 0)
    assert r.rc == 0, ih.name(r.rc)
    check_samples(r, xs, big_endian)
    assert r.ck == [1] * NSEQ
    assert r.model_n == N and r.model[:N].tobytes() == model.tobytes()
    assert ih.guards_intact(r)
    ih.same_as_strided(eng, kind, frames, r, N)


def test_chunks_hand_the_model_over(eng, sequence):
    """CMP_GPU_OPT_IMAGE_CHUNK so that chunks hold one frame, then up to five:
    byte-identical to the default (one chunk), with the caller's model buffer
    and with the engine's own."""
    kind, frames, xs, model = sequence
    offs, size = ih.back_to_back(frames)
    img = ih.place(frames, offs, size, 0)
    want = ih.run_image(eng, kind, img, offs, phase=3)
    assert want.rc == 0
    check_samples(want, xs)
    row = (2 * N + 15) // 16 * 16
    five = 5 * (row + (max(len(f) for f in frames) + 15) // 16 * 16)
    for budget in (1, five):
        counts = ih.plan([len(f) for f in frames], [N] * NSEQ, budget)
        assert counts == [1] * NSEQ if budget == 1 else (len(counts) > 1 and min(counts[:-1]) >= 5), counts
        try:
            assert eng.set_option(pkg.OPT_IMAGE_CHUNK, budget) == 0
            got = ih.run_image(eng, kind, img, offs, phase=3)
            own = ih.run_image(eng, kind, img, offs, phase=3, want_model=False)
        finally:
            assert eng.set_option(pkg.OPT_IMAGE_CHUNK, 0) == 0
        for r in (got, own):
            assert r.rc == 0 and r.dof == want.dof and r.status == want.status and r.ck == want.ck, budget
            assert np.array_equal(r.out, want.out), budget
            assert ih.guards_intact(r)
        assert got.model_n == N and np.array_equal(got.model, want.model), budget
        assert got.model[:N].tobytes() == model.tobytes()


def test_table_order_not_address_order(eng, sequence):
    """The same frames at shuffled places of the image, gaps of junk between
    them, the table in sequence order."""
    kind, frames, xs, model = sequence
    rng = np.random.default_rng(7)
    order = rng.permutation(NSEQ)
    offs, pos = [0] * NSEQ, 3
    for f in order:
        offs[f] = pos
        pos += len(frames[f]) + int(rng.integers(0, 23))
    assert offs != sorted(offs)
    r = ih.run_image(eng, kind, ih.place(frames, offs, pos + 9, 0xC3), offs, phase=9)
    assert r.rc == 0
    check_samples(r, xs)
    assert r.ck == [1] * NSEQ and r.model_n == N and r.model[:N].tobytes() == model.tobytes()
    ih.same_as_strided(eng, kind, frames, r, N)


def test_gather_shaped_table(eng, mixed):
    """The layout cmp_gpu_pack_frames leaves: 8-byte aligned offsets from the
    device, the bytes between the frames 0xFF."""
    import torch
    frames, xs = mixed
    nf = len(frames)
    cap = (max(len(f) for f in frames) + 7) // 8 * 8
    rows = np.full(nf * cap, 0xFF, dtype=np.uint8)
    for i, f in enumerate(frames):
        rows[i * cap:i * cap + len(f)] = np.frombuffer(f, dtype=np.uint8)
    d_rows = torch.from_numpy(rows).cuda()
    sizes = torch.tensor([len(f) for f in frames], dtype=torch.int32, device="cuda")
    packed = torch.full((nf * cap,), 0xFF, dtype=torch.uint8, device="cuda")
    d_offs = torch.zeros(nf + 1, dtype=torch.int64, device="cuda")
    assert eng.pack_frames(d_rows.data_ptr(), cap, cap, sizes.data_ptr(), nf, packed.data_ptr(), d_offs.data_ptr()) == 0
    assert eng.synchronize() == 0
    offs = [int(o) for o in d_offs.cpu().numpy()]
    assert all(o % 8 == 0 for o in offs) and any(len(f) % 8 for f in frames)
    img = packed.cpu().numpy()[:offs[-1]]
    for f, o in zip(frames, offs):
        gap = img[o + len(f):o + (len(f) + 7) // 8 * 8]
        assert (gap == 0xFF).all()
    r = ih.run_image(eng, "u16", img, offs[:-1])
    assert r.rc == 0
    check_samples(r, xs)
    ih.same_as_strided(eng, "u16", frames, r, max(SIZES))


@pytest.fixture(scope="module")
def plain(orc):
    """8 independent DIFF frames of 500 samples with checksums."""
    rng = np.random.default_rng(55)
    prm = api.CmpParams(primary_preprocessing=ih.DIFF, primary_encoder_type=ih.GOLOMB_ZERO, primary_encoder_param=16,
                        checksum_enabled=1)
    frames, xs, _ = ih.oracle_sequence(orc, prm, "u16", 500, rng, 8)
    return frames, xs


@pytest.mark.parametrize("what", ["cut short", "size below 16", "odd original size"])
def test_unusable_slices_stay_local(eng, plain, what):
    frames, xs = plain
    frames = list(frames)
    nf = len(frames)
    offs, size = ih.back_to_back(frames)
    k = nf - 1 if what == "cut short" else 3
    strided = list(frames)
    if what == "cut short":
        size -= 5
        strided[k] = bytes(24)  # for the strided call: a row without a frame
    else:
        b = bytearray(frames[k])
        if what == "size below 16":
            b[2:5] = (15).to_bytes(3, "big")
        else:
            b[5:8] = (2 * 500 - 1).to_bytes(3, "big")
        frames[k] = strided[k] = bytes(b)
    img = ih.place(frames, offs, size + 5, 0)[:size]
    r = ih.run_image(eng, "u16", img, offs, phase=11)
    assert r.rc == 0
    want_dof = [0]
    for f in range(nf):
        want_dof.append(want_dof[-1] + (0 if f == k else 1000))
    assert r.dof == want_dof
    assert ih.name(r.status[k]) == "INT_HDR"
    check_samples(r, xs, which=set(range(nf)) - {k})
    assert r.ck == [0 if f == k else 1 for f in range(nf)]
    assert ih.guards_intact(r)
    ih.same_as_strided(eng, "u16", strided, r, 500)


def test_damage_stays_in_its_frame(eng, plain):
    frames, xs = plain
    nf = len(frames)
    offs, size = ih.back_to_back(frames)
    # one payload bit of frame 2
    bad = list(frames)
    b = bytearray(bad[2])
    b[22 + 40] ^= 0x08
    bad[2] = bytes(b)
    r = ih.run_image(eng, "u16", ih.place(bad, offs, size, 0), offs, phase=1)
    assert r.rc == 0 and r.dof == [1000 * f for f in range(nf + 1)]
    check_samples(r, xs, which=set(range(nf)) - {2})
    assert api.is_error(r.status[2]) or r.ck[2] == 2
    assert [c for f, c in enumerate(r.ck) if f != 2] == [1] * (nf - 1)
    assert ih.guards_intact(r)
    ih.same_as_strided(eng, "u16", bad, r, 500)
    # one checksum byte of frame 5
    bad = list(frames)
    b = bytearray(bad[5])
    b[-3] ^= 0x40
    bad[5] = bytes(b)
    r = ih.run_image(eng, "u16", ih.place(bad, offs, size, 0), offs, phase=1)
    assert r.rc == 0
    check_samples(r, xs)
    assert r.ck == [2 if f == 5 else 1 for f in range(nf)]
    ih.same_as_strided(eng, "u16", bad, r, 500)


def test_capacity_one_byte_short(eng, plain):
    frames, xs = plain
    offs, size = ih.back_to_back(frames)
    r = ih.run_image(eng, "u16", ih.place(frames, offs, size, 0), offs, capacity_delta=-1)
    assert ih.name(r.rc) == "DST_TOO_SMALL"
    assert r.dof[-1] == 1000 * len(frames)  # the layout is still reported
    assert (r.out == r.fill).all() and ih.guards_intact(r)
    assert r.status == [0x5A5A5A5A] * len(frames)


def test_model_too_small_is_refused(eng, plain):
    frames, xs = plain
    offs, size = ih.back_to_back(frames)
    r = ih.run_image(eng, "u16", ih.place(frames, offs, size, 0), offs, nmodel=499)
    assert ih.name(r.rc) == "GENERIC"
    assert (r.out == r.fill).all() and r.status == [0x5A5A5A5A] * len(frames)
