"""Helpers of the image decoder's tests (cmp_gpu_decompress_image).  Truth is
the encoder: frames come from the CPU oracle's call loop and the expected
output is the source samples' low 16 bits.  make_x / low16 / oracle_sequence
restate tests/test_gpu_decode_seq.py's."""
import numpy as np

from conftest import load_pkg

pkg = load_pkg()
api = pkg.cmpapi

NONE, DIFF, IWT, MODEL = 0, 1, 2, 3
UNCOMPRESSED, GOLOMB_ZERO, GOLOMB_MULTI = 0, 1, 2


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


def oracle_sequence(orc, params, kind, n, rng, fpc, noisy=(), step=300):
    """One context's frames from the oracle's call loop: (frames, inputs' low
    halves, the model it holds at the end or None).  The acquisitions share a
    random walk of +-step per sample; the noisy ones do not compress."""
    ctx = api.CmpContext()
    wbs = orc.cal_work_buf_size(params, (4 if kind == "i16_in_i32" else 2) * n)
    assert not api.is_error(wbs), api.error_name(wbs)
    wb = api.aligned_empty(max(wbs, 2), fill=0)
    assert not api.is_error(orc.initialise(ctx, params, wb if wbs else None, wbs))
    base = np.cumsum(rng.integers(-step, step + 1, n)) + int(rng.integers(0, 1 << 16))
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


def name(s):
    return api.error_name(s) if api.is_error(s) else s


def walk(blob):
    """The Python form of cmp_gpu_frame_table: (offsets, bad_at or None)."""
    offs, pos = [], 0
    while pos < len(blob):
        if len(blob) - pos < 16:
            return offs, pos
        fs = int.from_bytes(blob[pos + 2:pos + 5], "big")
        if fs < 16 or fs > len(blob) - pos:
            return offs, pos
        offs.append(pos)
        pos += fs
    return offs, None


def place(frames, offsets, size, fill):
    """An image of `size` bytes of `fill` with frame i at offsets[i]."""
    img = np.full(size, fill, dtype=np.uint8)
    for f, o in zip(frames, offsets):
        img[o:o + len(f)] = np.frombuffer(f, dtype=np.uint8)
    return img


def back_to_back(frames):
    offs = np.concatenate([[0], np.cumsum([len(f) for f in frames])]).astype(np.int64)
    return [int(o) for o in offs[:-1]], int(offs[-1])


class Result:
    pass


def run_image(eng, kind, img, offsets, phase=0, flags=0, want_model=True, want_ck=True, nmodel=None,
              capacity_delta=0, guard=64, fill=0x5A):
    """Upload `img` at byte phase `phase` of a larger tensor whose other bytes
    are 0xA5, decode it, and return statuses, the output with its guards, the
    offsets, checksum_ok, model and model_n."""
    import torch
    img = np.asarray(img, dtype=np.uint8)
    nf = len(offsets)
    big = np.full(img.size + 64 + 64, 0xA5, dtype=np.uint8)
    big[16 + phase:16 + phase + img.size] = img
    src = torch.from_numpy(big).cuda()
    assert src.data_ptr() % 16 == 0
    total = 0
    for o in offsets:  # what the headers promise, for the output's size
        if o + 16 <= img.size:
            cs = int.from_bytes(bytes(img[o + 2:o + 5]), "big")
            osz = int.from_bytes(bytes(img[o + 5:o + 8]), "big")
            if cs >= 16 and o + cs <= img.size and osz % 2 == 0:
                total += osz
    nmodel = nmodel or max(total // 2, 1)
    dst = torch.full((guard + total + guard + 2,), fill, dtype=torch.uint8, device="cuda")
    st = torch.full((nf,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    ck = torch.full((nf,), 77, dtype=torch.uint8, device="cuda")
    mod = torch.zeros(nmodel, dtype=torch.int16, device="cuda")
    mn = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rc, dof = eng.decompress_image(kind, src.data_ptr() + 16 + phase, img.size, offsets, dst.data_ptr() + guard,
                                   total + capacity_delta, st.data_ptr(), ck.data_ptr() if want_ck else 0,
                                   mod.data_ptr() if want_model else 0, nmodel if want_model else 0,
                                   mn.data_ptr() if want_model else 0, flags)
    assert eng.synchronize() == 0
    r = Result()
    r.rc = rc
    r.dof = [int(v) for v in dof]
    r.total = total
    r.status = [int(s) & 0xFFFFFFFF for s in st.cpu().numpy()]
    raw = dst.cpu().numpy()
    r.guards = (raw[:guard], raw[guard + total:])
    r.out = raw[guard:guard + total]
    r.ck = [int(v) for v in ck.cpu().numpy()]
    r.model = mod.cpu().numpy().view(np.uint16)
    r.model_n = int(mn.cpu().numpy()[0])
    r.fill = fill
    return r


def frame_samples(r, f, big_endian=False):
    b = r.out[r.dof[f]:r.dof[f + 1]]
    return b.view(">u2").astype(np.uint16) if big_endian else b.view(np.uint16)


def guards_intact(r):
    return bool((r.guards[0] == r.fill).all() and (r.guards[1] == r.fill).all())


def run_strided(eng, kind, frames, nmax, want_ck=True):
    """The same frames as one context of a strided cmp_gpu_decompress_sequences
    call: (rc, statuses, rows, model, model_n, checksum_ok)."""
    import torch
    cap = (max(24, max(len(f) for f in frames)) + 7) // 8 * 8
    nf = len(frames)
    host = np.zeros(nf * cap, dtype=np.uint8)
    for i, f in enumerate(frames):
        host[i * cap:i * cap + len(f)] = np.frombuffer(f, dtype=np.uint8)
    src = torch.from_numpy(host).cuda()
    dstride = 2 * nmax
    dst = torch.zeros(nf * dstride + 16, dtype=torch.uint8, device="cuda")
    st = torch.zeros(nf, dtype=torch.int32, device="cuda")
    mod = torch.zeros(nmax, dtype=torch.int16, device="cuda")
    mn = torch.zeros(1, dtype=torch.int32, device="cuda")
    ck = torch.full((nf,), 77, dtype=torch.uint8, device="cuda")
    rc = eng.decompress_sequences(kind, src.data_ptr(), cap, cap, 1, nf, dst.data_ptr(), dstride, nmax,
                                  st.data_ptr(), mod.data_ptr(), dstride, mn.data_ptr(),
                                  ck.data_ptr() if want_ck else 0, 0)
    assert eng.synchronize() == 0
    out = dst.cpu().numpy()
    rows = [out[i * dstride:(i + 1) * dstride].view(np.uint16) for i in range(nf)]
    return (rc, [int(s) & 0xFFFFFFFF for s in st.cpu().numpy()], rows, mod.cpu().numpy().view(np.uint16),
            int(mn.cpu().numpy()[0]), [int(v) for v in ck.cpu().numpy()])


def same_as_strided(eng, kind, frames, r, nmax):
    """Statuses, checksum_ok, model and model_n of an image call against the
    strided one-context call over the same frames."""
    rc, status, _, model, model_n, ck = run_strided(eng, kind, frames, nmax)
    assert rc == 0 and r.rc == 0, (name(rc), name(r.rc))
    assert [name(s) for s in r.status] == [name(s) for s in status]
    assert r.ck == ck
    assert r.model_n == model_n
    assert np.array_equal(r.model[:model_n], model[:model_n])


def plan(sizes, ns, budget):
    """The chunk rule of cmp_image_plan_next (csrc/cmp_image_plan.c) restated:
    the frame counts of the chunks."""
    def up16(v):
        return (v + 15) // 16 * 16
    counts, first = [], 0
    while first < len(sizes):
        cap, nmax, count = 32, max(ns[first - 1] if first else 1, 1), 0
        for f in range(first, len(sizes)):
            ncap, nn = max(cap, up16(sizes[f])), max(nmax, ns[f])
            if count == 65535 or (count and (count + 1) * (ncap + up16(2 * nn)) > budget):
                break
            cap, nmax, count = ncap, nn, count + 1
        counts.append(count)
        first += count
    return counts
