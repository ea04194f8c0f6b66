#!/usr/bin/env python3
"""encode_kernel micro-benchmark (the kernel has no bench.py workload): the
cfg2 samples with g = 256 (k = 8, past the Rice kernel), as
  frames  16 frames x 4 Mi u16, DIFF + GOLOMB_ZERO g=256 (cmp_gpu_compress)
  stream  one 64 Mi-sample stream, the same coder (cmp_gpu_encode_stream)
timed as kbench.py does: 5 spans of 20 back-to-back launches, one HIP event
pair each, over ROT rotated buffer sets (cold reads).  The launch counters
must show encode_kernel launches only.  Prints one JSON line per case.
usage: encode_kbench.py [frames|stream ...]"""
import ctypes
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402

G, ROT, SPANS, PER_SPAN = 256, 3, 5, 20
STATS = ("rice_lb1", "rice_lb0", "rice_stream", "rice_auto", "encode", "encode_stream",
         "decode_round")  # airs_dev.h airs_launch_stat
pkg = bench.load_pkg()
api = pkg.cmpapi
lib = pkg.load()
wl = bench.WORKLOADS["cfg2"]
stream = torch.cuda.current_stream()
eng = lib.engine(stream.cuda_stream)
n, nf = wl["n"], wl["fpc"]
stride = 2 * n
srcs = [torch.empty(nf * stride, dtype=torch.uint8, device="cuda") for _ in range(ROT)]
for src in srcs:
    for j, f in enumerate(bench.frame_ids(wl, 0, 1)):
        eng.synthesize(src.data_ptr() + j * stride, 2, wl["seed"], f, n, 1, stride, bench.noise_w(wl, f))
cap = lib.compress_bound(2 * n)
cap = cap if not api.is_error(cap) else 3 * 2 * n + 64  # (the bound is an error past the 24-bit size field)
dstride = (cap + 7) // 8 * 8
dsts = [torch.empty(nf * dstride, dtype=torch.uint8, device="cuda") for _ in range(ROT)]
sizes = torch.zeros(nf, dtype=torch.int32, device="cuda")
ctxs = pkg.context_array(1)
lib.initialise(ctxs[0], api.CmpParams(**dict(wl["params"], primary_encoder_param=G)))


def launch_stats():
    out = (ctypes.c_uint64 * len(STATS))()
    fn = lib.lib.airs_dev_launch_stats
    fn.argtypes = [ctypes.POINTER(ctypes.c_uint64), ctypes.c_uint32]
    fn.restype = ctypes.c_uint32
    assert fn(out, len(STATS)) == len(STATS)
    return [int(v) for v in out]


def launch(case, k):
    src, dst = srcs[k % ROT], dsts[k % ROT]
    if case == "stream":
        r = eng.encode_stream("u16", src.data_ptr(), nf * n, wl["params"]["primary_preprocessing"],
                              wl["params"]["primary_encoder_type"], G, 0, dst.data_ptr(), nf * dstride - 64,
                              sizes.data_ptr())
    else:
        r = eng.compress(ctxs, nf, "u16", src.data_ptr(), stride, stride, dst.data_ptr(), dstride, cap,
                         sizes.data_ptr(), 0)
    assert r == 0, api.error_name(r)


for case in sys.argv[1:] or ["frames", "stream"]:
    before = launch_stats()
    for k in range(10):
        launch(case, k)
    torch.cuda.synchronize()
    ms = []
    for rep in range(SPANS):
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for k in range(PER_SPAN):
            launch(case, k)
        e1.record(stream)
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / PER_SPAN)
    assert eng.synchronize() == 0
    took = {s: a - b for s, a, b in zip(STATS, launch_stats(), before) if a != b}
    assert took == {"encode_stream" if case == "stream" else "encode": 10 + SPANS * PER_SPAN}, took
    sz = sizes.cpu().numpy()
    print(json.dumps(dict(case=case, g=G, rot=ROT, spans_ms=[round(m, 5) for m in ms],
                          mean_ms=round(sum(ms) / len(ms), 5), min_ms=round(min(ms), 5),
                          GBps=round(nf * 2 * n / (sum(ms) / len(ms) * 1e-3) / 1e9, 1),
                          bytes_out=int(sz[0]) if case == "stream" else int(sz.astype("int64").sum()))), flush=True)
eng.close()
