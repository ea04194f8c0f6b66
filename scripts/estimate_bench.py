#!/usr/bin/env python3
"""Cost of sizing frames under sixteen parameter sets in one call
(cmp_gpu_estimate) against what a caller had to do for the same answers
before: sixteen cmp_gpu_compress calls, one per parameter set, of which only
sizes[] is read; and, for the Rice list, against the selection kernel of
CMP_GPU_AUTO_RICE alone (airs_dev_select_rice), which answers less (a choice,
no sizes) from a 129-bin histogram.

Workload: cfg2's shape, 16 frames of 4 Mi u16 samples of the counter-hash
signal, and two candidate lists:

    rice    the sixteen GOLOMB_ZERO g = 2^k under DIFF
    mixed   sixteen candidates: NONE / DIFF, ZERO / MULTI, general g

Five variants, interleaved, on one box.  Every call is cold: the input sets
rotate (SETS x 128 MiB, more than the 256 MiB Infinity Cache between two uses
of a set) and a buffer larger than the cache is rewritten before each call.
HIP events around the call; WARMUP untimed rounds of every variant first
(code objects, engine scratch); median and min-max of REPS repeats.  The
sixteen compress calls of one repeat read the same set, as a caller's would:
only the first of them is cold.  The warm-up checks the variants against each
other: every frame size follows from the estimate's bits
(cmp_gpu_estimate_frame_size), and best is the selection kernel's k.

    python scripts/estimate_bench.py --out profiles/estimate_time.json
"""
import argparse
import ctypes
import importlib.util
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "airs-compression_amd")
FRAMES, N, SETS, WARMUP = 16, 4 << 20, 4, 2
NONE, DIFF = 0, 1
ZERO, MULTI = 1, 2
RICE = [(DIFF, ZERO, 1 << k, 0) for k in range(16)]
MIXED = [(DIFF, ZERO, 24, 0), (DIFF, ZERO, 32, 0), (DIFF, ZERO, 40, 0), (DIFF, ZERO, 48, 0), (NONE, ZERO, 1000, 0),
         (NONE, ZERO, 3000, 0), (DIFF, MULTI, 24, 100), (DIFF, MULTI, 32, 200), (DIFF, MULTI, 40, 300),
         (DIFF, MULTI, 12, 60), (NONE, MULTI, 2048, 20000), (NONE, MULTI, 1500, 9000), (DIFF, ZERO, 20, 0),
         (DIFF, ZERO, 28, 0), (DIFF, MULTI, 20, 150), (DIFF, MULTI, 28, 250)]
VARIANTS = ("estimate_rice", "estimate_mixed", "compress16_rice", "compress16_mixed", "select_rice")


def load_pkg():
    spec = importlib.util.spec_from_file_location("airs_compression_amd", os.path.join(PKG_DIR, "__init__.py"),
                                                  submodule_search_locations=[PKG_DIR])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["airs_compression_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    pkg = load_pkg()
    api = pkg.cmpapi
    lib = pkg.load()
    assert lib.gpu_available(), "no HIP device"
    eng = lib.engine()
    dev = ctypes.cast(eng.handle, ctypes.POINTER(ctypes.c_void_p))[0]  # struct cmp_gpu_engine: the device engine first
    select = lib.lib.airs_dev_select_rice
    select.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32,
                       ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                       ctypes.c_void_p]
    select.restype = ctypes.c_uint32

    fb = 2 * N
    sets = [torch.empty(FRAMES * N, dtype=torch.int16, device="cuda") for _ in range(SETS)]
    for s in sets:  # the same samples in every set
        assert eng.synthesize(s.data_ptr(), 2, 0xA1A6, 0, N, FRAMES, fb, 32) == 0
    cap = 3 * fb + 64
    stride = (cap + 7) // 8 * 8
    dst = torch.zeros(FRAMES * stride, dtype=torch.uint8, device="cuda")
    sizes = torch.zeros(16 * FRAMES, dtype=torch.int32, device="cuda")
    bits = {"rice": torch.zeros(FRAMES * 16, dtype=torch.int64, device="cuda"),
            "mixed": torch.zeros(FRAMES * 16, dtype=torch.int64, device="cuda")}
    best = torch.zeros(FRAMES, dtype=torch.int32, device="cuda")
    out_g = torch.zeros(FRAMES, dtype=torch.int32, device="cuda")
    flush = torch.empty(512 << 20, dtype=torch.uint8, device="cuda")
    lists = {"rice": RICE, "mixed": MIXED}
    arrays = {k: pkg.candidate_array(v) for k, v in lists.items()}
    ctxs = {k: [pkg.context_array(1) for _ in v] for k, v in lists.items()}
    turn = [0]

    def estimate(which):
        def call(src):
            rc = eng.estimate("u16", src, fb, fb, FRAMES, arrays[which], bits[which].data_ptr(), best.data_ptr())
            assert rc == 0, api.error_name(rc)
        return call

    def compress16(which):
        def call(src):
            for c, (pre, enc, g, outl) in enumerate(lists[which]):
                ctx = ctxs[which][c]
                prm = api.CmpParams(primary_preprocessing=pre, primary_encoder_type=enc, primary_encoder_param=g,
                                    primary_encoder_outlier=outl)
                assert not api.is_error(lib.initialise(ctx[0], prm))
                rc = eng.compress(ctx, FRAMES, "u16", src, fb, fb, dst.data_ptr(), stride, cap,
                                  sizes.data_ptr() + 4 * FRAMES * c)
                assert rc == 0, api.error_name(rc)
        return call

    def select_rice(src):
        assert select(dev, src, fb, 2, N, FRAMES, None, 0, 1, DIFF, out_g.data_ptr()) == 0

    calls = {"estimate_rice": estimate("rice"), "estimate_mixed": estimate("mixed"),
             "compress16_rice": compress16("rice"), "compress16_mixed": compress16("mixed"),
             "select_rice": select_rice}

    def timed(fn):
        src = sets[turn[0] % SETS].data_ptr()
        turn[0] += 1
        flush.fill_(1)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(src)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3  # us

    # warm up every variant, then check them against each other
    for _ in range(WARMUP):
        for name in VARIANTS:
            timed(calls[name])
    checked = skipped = 0
    for which in ("rice", "mixed"):
        calls["estimate_" + which](sets[0].data_ptr())
        calls["compress16_" + which](sets[0].data_ptr())
        assert eng.synchronize() == 0
        b = bits[which].cpu().numpy().reshape(FRAMES, 16)
        sz = sizes.cpu().numpy().astype(np.uint32).reshape(16, FRAMES)
        for c, cand in enumerate(lists[which]):
            for f in range(FRAMES):
                if api.is_error(int(sz[c, f])):  # a frame the encoder refuses (the 24-bit size field)
                    skipped += 1
                    continue
                assert lib.estimate_frame_size(cand, int(b[f, c]), 0) == int(sz[c, f]), (which, c, f)
                checked += 1
        if which == "rice":
            select_rice(sets[0].data_ptr())
            assert eng.synchronize() == 0
            assert (1 << best.cpu().numpy().astype(np.int64) == out_g.cpu().numpy()).all()
            rice_best = best.cpu().numpy().tolist()
    t = {name: [] for name in VARIANTS}
    for _ in range(a.reps):
        for name in VARIANTS:
            t[name].append(timed(calls[name]))
    res = {
        "workload": {"frames": FRAMES, "samples_per_frame": N, "sample_bytes": FRAMES * fb, "candidates": 16,
                     "rice": RICE, "mixed": MIXED, "cold": True, "input_sets": SETS, "warmup_rounds": WARMUP,
                     "reps": a.reps, "frame_sizes_checked": checked, "frames_the_encoder_refused": skipped,
                     "rice_best_k": rice_best},
    }
    for name in VARIANTS:
        res[name + "_us"] = {"median": statistics.median(t[name]), "min": min(t[name]), "max": max(t[name]),
                             "all": t[name]}
    for which in ("rice", "mixed"):
        res[f"compress16_{which}_over_estimate_{which}"] = (res[f"compress16_{which}_us"]["median"] /
                                                           res[f"estimate_{which}_us"]["median"])
    res["estimate_rice_over_select_rice"] = res["estimate_rice_us"]["median"] / res["select_rice_us"]["median"]
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
