"""Helpers of the image encoder's tests (cmp_gpu_compress_image).  A case is a
sample image (bytes), a table of (offset, frame_bytes) into it, a sample type
and whether the samples are big-endian.  Truth is the CPU oracle's call loop
over the table, frame by frame, with the same timestamp function: the sizes,
the concatenated frames (the expected .air image), the context's fields and
the work buffer."""
import numpy as np

from conftest import load_pkg

pkg = load_pkg()
api = pkg.cmpapi

NONE, DIFF, IWT, MODEL = 0, 1, 2, 3
UNCOMPRESSED, GOLOMB_ZERO, GOLOMB_MULTI = 0, 1, 2
GUARD = 64
FILL = 0xAB
TOO_SMALL = api.err_value("DST_TOO_SMALL")


def ts_counter(start):
    stamp = [start]

    def ts():
        stamp[0] += 1
        return (stamp[0] >> 16, stamp[0] & 0xFFFF)
    return ts


def sample_bytes(kind):
    return 4 if kind == "i16_in_i32" else 2


def native(img, off, fb, kind, big_endian):
    """Frame (off, fb) of the image as the array the loop's call takes: native
    samples where fb is a whole number of them, else the bytes."""
    b = np.ascontiguousarray(img[off:off + fb])
    if fb == 0 or fb % sample_bytes(kind):
        return b
    if kind == "i16_in_i32":
        return b.view(np.int32).copy()
    x = b.view(">u2" if big_endian else "<u2").astype(np.uint16)
    return x if kind == "u16" else x.view(np.int16)


def work_size(lib, params, fbs):
    w = lib.cal_work_buf_size(params, max(max(fbs), 2))
    return 0 if api.is_error(w) else w


class Result:
    pass


def truth(orc, params, kind, img, offs, fbs, big_endian=False, wbs=None, primary_g=None, ts_start=7000):
    """The loop of include/cmp_gpu.h over the table."""
    wbs = work_size(orc, params, fbs) if wbs is None else wbs
    r = Result()
    orc.set_timestamp_func(ts_counter(ts_start))
    try:
        ctx = api.CmpContext()
        wb = api.aligned_empty(max(wbs, 2), fill=0)
        e = orc.initialise(ctx, params, wb if wbs else None, wbs)
        assert not api.is_error(e), api.error_name(e)
        r.sizes, r.frames = [], []
        for o, fb in zip(offs, fbs):
            x = native(img, int(o), int(fb), kind, big_endian)
            cap = orc.compress_bound(int(fb))
            dst = api.aligned_empty(max(cap if not api.is_error(cap) else 0, 64))
            if primary_g is not None:
                ctx.params.primary_encoder_param = primary_g(x)
            s = orc.compress(kind, ctx, dst, cap, x if x.size else dst, int(fb)) & 0xFFFFFFFF
            r.sizes.append(s)
            r.frames.append(None if api.is_error(s) else bytes(dst[:s]))
        r.state = (ctx.identifier, ctx.sequence_number, ctx.model_size)
        r.work = bytes(wb[:wbs])
    finally:
        orc.set_timestamp_func(None)
    r.image = b"".join(f for f in r.frames if f is not None)
    r.offsets = [0]
    for f in r.frames:
        r.offsets.append(r.offsets[-1] + (len(f) if f is not None else 0))
    return r


def cut(t, capacity):
    """What the call leaves of truth t at out_capacity `capacity`: the first
    frame that does not fit and every frame after it CMP_ERR_DST_TOO_SMALL."""
    r = Result()
    r.state, r.work = t.state, t.work
    r.sizes, r.offsets, stuck = [], [0], False
    for s in t.sizes:
        take = 0 if api.is_error(s) else s
        stuck = stuck or r.offsets[-1] + take > capacity
        r.sizes.append(TOO_SMALL if stuck else s)
        r.offsets.append(r.offsets[-1] + (0 if stuck else take))
    r.image = t.image[:r.offsets[-1]]
    return r


def launch(prod, eng, params, kind, img, offs, fbs, big_endian=False, wbs=None, batch_flags=0, capacity=None,
           total=None, src_phase=0, out_phase=0, ts_start=7000):
    """Queue one cmp_gpu_compress_image call: the image at byte phase src_phase
    of a 16-byte aligned tensor whose other bytes are 0xA5, the output at byte
    phase out_phase of a tensor of 0xAB.  `total`: the bytes the full result
    takes (sizes the output; `capacity` defaults to it).  Nothing waits."""
    import torch
    img = np.asarray(img, dtype=np.uint8)
    nf = len(offs)
    wbs = work_size(prod, params, fbs) if wbs is None else wbs
    capacity = total if capacity is None else capacity
    h = Result()
    big = np.full(16 + 16 + img.size + 64, 0xA5, dtype=np.uint8)
    big[16 + src_phase:16 + src_phase + img.size] = img
    h.src = torch.from_numpy(big).cuda()
    assert h.src.data_ptr() % 16 == 0
    h.out = torch.full((GUARD + 16 + max(total, capacity) + 2 * GUARD,), FILL, dtype=torch.uint8, device="cuda")
    assert h.out.data_ptr() % 16 == 0
    h.out_at = GUARD + out_phase
    h.capacity = capacity
    h.offs = torch.full((nf + 1,), -3, dtype=torch.int64, device="cuda")
    h.sizes = torch.full((nf,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    h.work = torch.zeros(max(wbs, 2) + 16, dtype=torch.uint8, device="cuda")
    h.wbs = wbs
    h.ctx = api.CmpContext()
    prod.set_timestamp_func(ts_counter(ts_start))
    try:
        e = prod.initialise(h.ctx, params, h.work.data_ptr() if wbs else None, wbs)
        assert not api.is_error(e), api.error_name(e)
        torch.cuda.synchronize()
        h.rc = eng.compress_image(h.ctx, kind, h.src.data_ptr() + 16 + src_phase, img.size, offs, fbs,
                                  h.out.data_ptr() + h.out_at, capacity, h.offs.data_ptr(), h.sizes.data_ptr(),
                                  batch_flags, pkg.IMG_SRC_BIG_ENDIAN if big_endian else 0)
    finally:
        prod.set_timestamp_func(None)
    return h


def collect(eng, h):
    assert h.rc == 0, api.error_name(h.rc)
    assert eng.synchronize() == 0
    r = Result()
    r.sizes = [int(s) & 0xFFFFFFFF for s in h.sizes.cpu().numpy()]
    r.offsets = [int(o) for o in h.offs.cpu().numpy()]
    raw = h.out.cpu().numpy()
    end = r.offsets[-1]
    assert 0 <= end <= h.capacity, (end, h.capacity)
    r.image = bytes(raw[h.out_at:h.out_at + end])
    # nothing before out, nothing from out_offsets[n] to 64 bytes past out_capacity
    r.guards = bool((raw[:h.out_at] == FILL).all() and
                    (raw[h.out_at + end:h.out_at + h.capacity + GUARD] == FILL).all())
    r.out_ptr = h.out.data_ptr() + h.out_at
    r.state = (h.ctx.identifier, h.ctx.sequence_number, h.ctx.model_size)
    r.work = bytes(h.work.cpu().numpy()[:h.wbs])
    return r


def run(prod, eng, params, kind, img, offs, fbs, **kw):
    return collect(eng, launch(prod, eng, params, kind, img, offs, fbs, **kw))


def stage_frames(prod):
    """The device layer's counters (airs_dev_encode_image_stats): frames that
    went through the ingest copy, frames handed to the emit copy, frames of
    refused runs, in this process so far."""
    import ctypes
    out = (ctypes.c_uint64 * 3)()
    fn = prod.lib.airs_dev_encode_image_stats
    fn.argtypes, fn.restype = [ctypes.c_void_p, ctypes.c_uint32], ctypes.c_uint32
    assert fn(out, 3) == 3
    return [int(v) for v in out]


def names(sizes):
    return [api.error_name(s) if api.is_error(s) else s for s in sizes]


def same(got, want, what=""):
    """Everything a call leaves, against the loop's."""
    assert names(got.sizes) == names(want.sizes), what
    assert got.offsets == want.offsets, what
    assert got.image == want.image, (what, first_difference(got.image, want.image))
    assert got.guards, (what, "written outside [out, out + out_offsets[n])")
    assert got.state == want.state, (what, got.state, want.state)
    assert got.work == want.work, (what, "work buffer")


def first_difference(a, b):
    n = min(len(a), len(b))
    d = np.nonzero(np.frombuffer(a[:n], dtype=np.uint8) != np.frombuffer(b[:n], dtype=np.uint8))[0]
    return (len(a), len(b), int(d[0]) if d.size else None)


def smooth(rng, n, step=12):
    """n native u16 samples of a random walk: they compress."""
    return ((30000 + np.cumsum(rng.integers(-step, step + 1, n))) & 0xFFFF).astype(np.uint16)


def stored(x, big_endian):
    """The bytes a sample file holds for the native 16-bit samples x."""
    x = np.ascontiguousarray(x).view(np.uint16)
    return (x.byteswap() if big_endian else x).view(np.uint8)


def place(chunks, phases, fill=0x5C):
    """An image with chunk i (bytes) at the next position whose byte phase is
    phases[i % len(phases)]: (image, offsets)."""
    parts, offs, pos = [], [], 0
    for i, c in enumerate(chunks):
        pad = (phases[i % len(phases)] - pos) % 16
        parts.append(np.full(pad, fill, dtype=np.uint8))
        offs.append(pos + pad)
        parts.append(np.asarray(c, dtype=np.uint8))
        pos += pad + len(c)
    return np.concatenate(parts), offs


def select_g(orc_ext, kind, pre):
    """The CMP_GPU_AUTO_RICE rule through the oracle: frame -> g = 2^k."""
    def g(x):
        return 1 << orc_ext.orc_select_rice_k(np.ascontiguousarray(x).ctypes.data, x.size,
                                              1 if kind == "i16_in_i32" else 0, pre, None)
    return g

