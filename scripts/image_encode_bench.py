#!/usr/bin/env python3
"""Cost of compressing a sample image (cmp_gpu_compress_image: ingest + encode
+ offset scan + emit) against the strided batch followed by the 8-byte pack
(cmp_gpu_compress + cmp_gpu_pack_frames) on the same samples pre-staged in
native rows.

Workload: FRAMES frames of N u16 samples of the counter-hash signal, DIFF +
GOLOMB_ZERO g = 32.  Four variants, interleaved, every call cold (a buffer
larger than the Infinity Cache is rewritten before it), HIP events around the
call, median and min-max of REPS repeats:

    batch_pack   cmp_gpu_compress over native rows + cmp_gpu_pack_frames
    image_direct the image call, native samples at an aligned constant stride
    image_odd    the image call, the same samples from an odd byte offset
    image_be     the image call, big-endian samples (the sample files' form)

Kernel times come from a profiler run of this script with --once VARIANT
(rocprofv3 --kernel-trace: the kernels after the last fill of the flush buffer
are the one cold call); profiles/image_encode.json holds them beside the table.

    python scripts/image_encode_bench.py --out profiles/image_encode.json

--ragged measures CMP_GPU_OPT_IMAGE_RAGGED under the same
discipline: 1024 u16 frames of 64 Ki + 2 i samples (every size differs), native
and aligned or big-endian, with the option off (1024 runs) and on; then, for
the built-in keep threshold, runs of 2 .. 1024 equal frames of 64 Ki samples on
the run path against the same frames in a ragged piece (option value
0xFFFFFFFF: no run is kept).  --once takes VARIANT names of that mode too.

    python scripts/image_encode_bench.py --ragged --out profiles/image_encode_ragged.json

--checksum measures CMP_GPU_OPT_IMAGE_RAGGED_CHECKSUM the
same way: the 1024 frames of 64 Ki + 2 i samples under a checksum-enabled
context, CMP_GPU_OPT_IMAGE_RAGGED on throughout, option 6 off (the context is
ineligible: 1024 runs with a checksum launch pair each) against option 6 on.

    python scripts/image_encode_bench.py --checksum --out profiles/image_encode_ragged_checksum.json
"""
import argparse
import importlib.util
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "airs-compression_amd")
FRAMES, N, G = 1024, 65536, 32
VARIANTS = ("batch_pack", "image_direct", "image_odd", "image_be")
RAGGED_VARIANTS = ("native_off", "native_on", "be_off", "be_on")
KEEP_RUNS = (2, 8, 32, 128, 1024)
NO_KEEP = 0xFFFFFFFF  # option value: on, and no run of equal frames is large enough to be kept


def load_pkg():
    spec = importlib.util.spec_from_file_location("airs_compression_amd", os.path.join(PKG_DIR, "__init__.py"),
                                                  submodule_search_locations=[PKG_DIR])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["airs_compression_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def stats(ts):
    return {"median": statistics.median(ts), "min": min(ts), "max": max(ts), "all": ts}


def ragged_main(a):
    """The ragged option's two measurements (module docstring)."""
    import torch
    pkg = load_pkg()
    api = pkg.cmpapi
    lib = pkg.load()
    assert lib.gpu_available(), "no HIP device"
    eng = lib.engine()
    ns = [N + 2 * i for i in range(FRAMES)]
    stride = (2 * ns[-1] + 15) // 16 * 16  # bytes between frames: every frame 16-byte aligned
    native = torch.empty(FRAMES * stride // 2 + 8, dtype=torch.int16, device="cuda")
    assert eng.synthesize(native.data_ptr(), 2, 0xA1A5, 0, stride // 2, FRAMES, stride, 32) == 0
    torch.cuda.synchronize()
    host = native.cpu().numpy()[:FRAMES * stride // 2].view(np.uint16)
    be = torch.from_numpy(host.byteswap().view(np.uint8).copy()).cuda()
    offs = np.arange(FRAMES, dtype=np.uint64) * stride
    fbs = np.array([2 * n for n in ns], dtype=np.uint32)
    eq_offs = np.arange(FRAMES, dtype=np.uint64) * (2 * N)  # the keep workload: equal frames, back to back
    eq_fbs = np.full(FRAMES, 2 * N, dtype=np.uint32)
    cap = lib.compress_bound(int(fbs[-1]))
    out = torch.zeros(FRAMES * cap, dtype=torch.uint8, device="cuda")
    ooffs = torch.zeros(FRAMES + 1, dtype=torch.int64, device="cuda")
    sizes = torch.zeros(FRAMES, dtype=torch.int32, device="cuda")
    flush = torch.empty(512 << 20, dtype=torch.uint8, device="cuda")
    prm = api.CmpParams(primary_preprocessing=1, primary_encoder_type=1, primary_encoder_param=G)
    ctxs = pkg.context_array(1)

    def image(src, flags, option, o, f, count=FRAMES):
        def call():
            assert eng.set_option(pkg.OPT_IMAGE_RAGGED, option) == 0
            rc = eng.compress_image(ctxs[0], "u16", src.data_ptr(), src.numel() * src.element_size(), o[:count],
                                    f[:count], out.data_ptr(), FRAMES * cap, ooffs.data_ptr(), sizes.data_ptr(), 0,
                                    flags)
            assert rc == 0, api.error_name(rc)
        call.count = count
        return call

    calls = {"native_off": image(native, 0, 0, offs, fbs), "native_on": image(native, 0, 1, offs, fbs),
             "be_off": image(be, pkg.IMG_SRC_BIG_ENDIAN, 0, offs, fbs),
             "be_on": image(be, pkg.IMG_SRC_BIG_ENDIAN, 1, offs, fbs)}
    for c in KEEP_RUNS:
        calls[f"run_{c}"] = image(native, 0, 0, eq_offs, eq_fbs, c)
        calls[f"ragged_{c}"] = image(native, 0, NO_KEEP, eq_offs, eq_fbs, c)

    def timed(fn):
        assert not api.is_error(lib.initialise(ctxs[0], prm))
        flush.fill_(1)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3  # us

    def frames_of(count):
        b, o, sz = out.cpu().numpy(), ooffs.cpu().numpy(), sizes.cpu().numpy().astype(np.int64)
        assert (sz[:count] > 0).all() and int(o[count]) == int(sz[:count].sum())
        return [bytes(b[int(o[f]):int(o[f]) + 8]) + bytes(b[int(o[f]) + 14:int(o[f]) + int(sz[f])])
                for f in range(count)], int(sz[:count].sum())

    # warm up, and the variants of a workload against each other: the same
    # frames, identifiers excepted (header bytes 8..13 come from the clock)
    want, total = {}, {}
    for name, fn in calls.items():
        for _ in range(2):
            assert not api.is_error(lib.initialise(ctxs[0], prm))
            fn()
        assert eng.synchronize() == 0
        key = "ragged" if name in RAGGED_VARIANTS else name.split("_")[1]
        got, total[key] = frames_of(fn.count)
        assert got == want.setdefault(key, got), f"{name} differs"
    if a.once:
        timed(calls[a.once])
        return
    res = {"workload": {"frames": FRAMES, "samples_per_frame": "65536 + 2 i", "preprocessing": "DIFF",
                        "encoder": "GOLOMB_ZERO", "g": G, "sample_bytes": int(fbs.sum()),
                        "compressed_bytes": total["ragged"], "cold": True, "reps": a.reps}}
    t = {name: [] for name in calls}
    for _ in range(a.reps):
        for name in RAGGED_VARIANTS:
            t[name].append(timed(calls[name]))
    for _ in range(a.reps):
        for name in calls:
            if name not in RAGGED_VARIANTS:
                t[name].append(timed(calls[name]))
    for name in RAGGED_VARIANTS:
        res[name + "_us"] = stats(t[name])
    for kind in ("native", "be"):
        off, on = res[kind + "_off_us"], res[kind + "_on_us"]
        res[kind + "_off_over_on"] = off["median"] / on["median"]
        res[kind + "_ranges_overlap"] = not (on["max"] < off["min"] or off["max"] < on["min"])
    res["keep"] = {"workload": "runs of equal frames of 65536 u16 samples, native and aligned", "runs": {}}
    for c in KEEP_RUNS:
        run, rag = stats(t[f"run_{c}"]), stats(t[f"ragged_{c}"])
        res["keep"]["runs"][str(c)] = {"sample_bytes": c * 2 * N, "run_path_us": run, "ragged_path_us": rag,
                                       "run_not_slower": run["median"] <= rag["median"],
                                       "ranges_overlap": not (run["max"] < rag["min"] or rag["max"] < run["min"])}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


def checksum_main(a):
    """Option 6 off against on under a checksum-enabled context (module docstring)."""
    import torch
    pkg = load_pkg()
    api = pkg.cmpapi
    lib = pkg.load()
    assert lib.gpu_available(), "no HIP device"
    eng = lib.engine()
    ns = [N + 2 * i for i in range(FRAMES)]
    stride = (2 * ns[-1] + 15) // 16 * 16  # bytes between frames: every frame 16-byte aligned
    native = torch.empty(FRAMES * stride // 2 + 8, dtype=torch.int16, device="cuda")
    assert eng.synthesize(native.data_ptr(), 2, 0xA1A5, 0, stride // 2, FRAMES, stride, 32) == 0
    torch.cuda.synchronize()
    host = native.cpu().numpy()[:FRAMES * stride // 2].view(np.uint16)
    be = torch.from_numpy(host.byteswap().view(np.uint8).copy()).cuda()
    offs = np.arange(FRAMES, dtype=np.uint64) * stride
    fbs = np.array([2 * n for n in ns], dtype=np.uint32)
    cap = lib.compress_bound(int(fbs[-1]))
    out = torch.zeros(FRAMES * cap, dtype=torch.uint8, device="cuda")
    ooffs = torch.zeros(FRAMES + 1, dtype=torch.int64, device="cuda")
    sizes = torch.zeros(FRAMES, dtype=torch.int32, device="cuda")
    flush = torch.empty(512 << 20, dtype=torch.uint8, device="cuda")
    prm = api.CmpParams(primary_preprocessing=1, primary_encoder_type=1, primary_encoder_param=G, checksum_enabled=1)
    ctxs = pkg.context_array(1)
    assert eng.set_option(pkg.OPT_IMAGE_RAGGED, 1) == 0

    def image(src, flags, option6):
        def call():
            assert eng.set_option(pkg.OPT_IMAGE_RAGGED_CHECKSUM, option6) == 0
            rc = eng.compress_image(ctxs[0], "u16", src.data_ptr(), src.numel() * src.element_size(), offs, fbs,
                                    out.data_ptr(), FRAMES * cap, ooffs.data_ptr(), sizes.data_ptr(), 0, flags)
            assert rc == 0, api.error_name(rc)
        return call

    calls = {"native_off": image(native, 0, 0), "native_on": image(native, 0, 1),
             "be_off": image(be, pkg.IMG_SRC_BIG_ENDIAN, 0), "be_on": image(be, pkg.IMG_SRC_BIG_ENDIAN, 1)}
    assert a.once is None or a.once in calls, a.once

    def timed(fn):
        assert not api.is_error(lib.initialise(ctxs[0], prm))
        flush.fill_(1)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3  # us

    # warm up, and the variants against each other: the same frames, checksums
    # included, identifiers excepted (header bytes 8..13 come from the clock)
    want, total = None, 0
    for name, fn in calls.items():
        for _ in range(2):
            assert not api.is_error(lib.initialise(ctxs[0], prm))
            fn()
        assert eng.synchronize() == 0
        b, o, sz = out.cpu().numpy(), ooffs.cpu().numpy(), sizes.cpu().numpy().astype(np.int64)
        assert (sz > 0).all() and int(o[FRAMES]) == int(sz.sum())
        got = [bytes(b[int(o[f]):int(o[f]) + 8]) + bytes(b[int(o[f]) + 14:int(o[f]) + int(sz[f])])
               for f in range(FRAMES)]
        assert all(g[15 - 6] & 8 for g in got), "checksum bit"
        want, total = want or got, int(sz.sum())
        assert got == want, f"{name} differs"
    if a.once:
        timed(calls[a.once])
        return
    res = {"workload": {"frames": FRAMES, "samples_per_frame": "65536 + 2 i", "preprocessing": "DIFF",
                        "encoder": "GOLOMB_ZERO", "g": G, "checksum_enabled": 1, "image_ragged": 1,
                        "sample_bytes": int(fbs.sum()), "compressed_bytes": total, "cold": True, "reps": a.reps}}
    t = {name: [] for name in calls}
    for _ in range(a.reps):
        for name in calls:
            t[name].append(timed(calls[name]))
    for name in calls:
        res[name + "_us"] = stats(t[name])
    for kind in ("native", "be"):
        off, on = res[kind + "_off_us"], res[kind + "_on_us"]
        res[kind + "_off_over_on"] = off["median"] / on["median"]
        res[kind + "_ranges_overlap"] = not (on["max"] < off["min"] or off["max"] < on["min"])
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out")
    ap.add_argument("--ragged", action="store_true", help="the CMP_GPU_OPT_IMAGE_RAGGED measurements")
    ap.add_argument("--once", help="warm up, then one cold call of this variant (for a profiler)")
    ap.add_argument("--checksum", action="store_true", help="the CMP_GPU_OPT_IMAGE_RAGGED_CHECKSUM measurements")
    a = ap.parse_args()
    if a.checksum:
        return checksum_main(a)
    if a.ragged:
        return ragged_main(a)
    assert a.once is None or a.once in VARIANTS, a.once
    import torch
    pkg = load_pkg()
    api = pkg.cmpapi
    lib = pkg.load()
    assert lib.gpu_available(), "no HIP device"
    eng = lib.engine()

    fb = 2 * N
    native = torch.empty(FRAMES * N + 8, dtype=torch.int16, device="cuda")
    assert eng.synthesize(native.data_ptr(), 2, 0xA1A5, 0, N, FRAMES, fb, 32) == 0
    torch.cuda.synchronize()
    host = native.cpu().numpy()[:FRAMES * N].view(np.uint16)
    odd = torch.from_numpy(np.concatenate([np.full(1, 0xA5, np.uint8), host.view(np.uint8),
                                           np.zeros(15, np.uint8)])).cuda()
    be = torch.from_numpy(host.byteswap().view(np.uint8).copy()).cuda()
    offs = (np.arange(FRAMES, dtype=np.uint64) * fb)
    fbs = np.full(FRAMES, fb, dtype=np.uint32)

    cap = lib.compress_bound(fb)
    stride = (cap + 7) // 8 * 8
    rows = torch.zeros(FRAMES * stride, dtype=torch.uint8, device="cuda")
    sizes = torch.zeros(FRAMES, dtype=torch.int32, device="cuda")
    packed = torch.zeros(FRAMES * stride, dtype=torch.uint8, device="cuda")
    poffs = torch.zeros(FRAMES + 1, dtype=torch.int64, device="cuda")
    out = torch.zeros(FRAMES * cap, dtype=torch.uint8, device="cuda")
    ooffs = torch.zeros(FRAMES + 1, dtype=torch.int64, device="cuda")
    flush = torch.empty(512 << 20, dtype=torch.uint8, device="cuda")
    prm = api.CmpParams(primary_preprocessing=1, primary_encoder_type=1, primary_encoder_param=G)
    ctxs = pkg.context_array(1)

    def fresh():
        assert not api.is_error(lib.initialise(ctxs[0], prm))

    def batch_pack():
        assert eng.compress(ctxs, FRAMES, "u16", native.data_ptr(), fb, fb, rows.data_ptr(), stride, cap,
                            sizes.data_ptr()) == 0
        assert eng.pack_frames(rows.data_ptr(), stride, cap, sizes.data_ptr(), FRAMES, packed.data_ptr(),
                               poffs.data_ptr()) == 0

    def image(src_ptr, flags):
        def call():
            rc = eng.compress_image(ctxs[0], "u16", src_ptr, FRAMES * fb, offs, fbs, out.data_ptr(), FRAMES * cap,
                                    ooffs.data_ptr(), sizes.data_ptr(), 0, flags)
            assert rc == 0, api.error_name(rc)
        return call

    calls = {"batch_pack": batch_pack, "image_direct": image(native.data_ptr(), 0),
             "image_odd": image(odd.data_ptr() + 1, 0), "image_be": image(be.data_ptr(), pkg.IMG_SRC_BIG_ENDIAN)}

    def timed(fn):
        fresh()
        flush.fill_(1)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3  # us

    # warm up (code objects, scratch) and check the variants against each other:
    # the same frames, identifiers excepted (header bytes 8..13 come from the clock)
    def frames_of(buf, o, sz):
        b = buf.cpu().numpy()
        return [bytes(b[int(o[f]):int(o[f]) + 8]) + bytes(b[int(o[f]) + 14:int(o[f]) + int(sz[f])])
                for f in range(FRAMES)]

    want = None
    for name in VARIANTS:
        for _ in range(2):
            fresh()
            calls[name]()
        assert eng.synchronize() == 0
        sz = sizes.cpu().numpy().astype(np.int64)
        assert (sz > 0).all() and (sz <= cap).all(), name
        got = frames_of(packed, poffs.cpu().numpy(), sz) if name == "batch_pack" else \
            frames_of(out, ooffs.cpu().numpy(), sz)
        if name != "batch_pack":
            assert int(ooffs[FRAMES]) == int(sz.sum()), name
        want = want or got
        assert got == want, f"{name} differs from batch_pack"
    total = int(sz.sum())
    if a.once:
        timed(calls[a.once])
        return
    t = {name: [] for name in VARIANTS}
    for _ in range(a.reps):
        for name in VARIANTS:
            t[name].append(timed(calls[name]))
    res = {
        "workload": {"frames": FRAMES, "samples_per_frame": N, "preprocessing": "DIFF", "encoder": "GOLOMB_ZERO",
                     "g": G, "sample_bytes": FRAMES * fb, "compressed_bytes": total, "cold": True, "reps": a.reps},
    }
    for name in VARIANTS:
        res[name + "_us"] = {"median": statistics.median(t[name]), "min": min(t[name]), "max": max(t[name]),
                             "all": t[name]}
    base = res["batch_pack_us"]
    for name in VARIANTS[1:]:
        res[name + "_over_batch_pack"] = res[name + "_us"]["median"] / base["median"]
    res["batch_pack_spread_us"] = base["max"] - base["min"]
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
