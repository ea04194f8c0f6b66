#!/usr/bin/env python3
"""Checksum-enabled encode: a bench workload with
checksum_enabled=1, timed per call with HIP events.  usage: ck_bench.py cfg2|cfg4

ck_bench.py ragged [OUT.json]: the ragged XXH32 (airs_dev_checksum_ragged,
DESIGN.md 3.4.6) against airs_dev_checksum on the same 1024 equal frames of
64 Ki u16 samples, in one process, interleaved, cold (512 MiB rewritten before
every call), HIP events around the call, 15 repeats; the two must give the
same checksums."""
import ctypes
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402

pkg = bench.load_pkg()
api = pkg.cmpapi
lib = pkg.load()
name = sys.argv[1] if len(sys.argv) > 1 else "cfg2"


class RaggedCk(ctypes.Structure):  # struct airs_ragged_ck (csrc/airs_dev.h)
    _fields_ = [("sample_bytes", ctypes.c_uint32), ("frames", ctypes.c_uint32), ("src", ctypes.c_void_p),
                ("n", ctypes.c_void_p), ("off", ctypes.c_void_p), ("bytes", ctypes.c_uint64),
                ("blocks", ctypes.c_void_p), ("num_blocks", ctypes.c_uint32), ("out", ctypes.c_void_p)]


def ragged_main(out_path):
    frames, n, reps = 1024, 65536, 15
    c = lib.lib
    eng = lib.engine()
    # struct cmp_gpu_engine (csrc/cmp_engine.h) begins with its airs_dev_engine pointer
    dev = ctypes.c_void_p.from_address(eng.handle if isinstance(eng.handle, int) else eng.handle.value).value
    src = torch.empty(frames * n, dtype=torch.int16, device="cuda")
    assert eng.synthesize(src.data_ptr(), 2, 0xA1A5, 0, n, frames, 2 * n, 32) == 0
    # the host's layout (cmp_image_plan.c): offsets, total, product workgroups
    fbs = np.full(frames, 2 * n, dtype=np.uint32)
    off = np.zeros(frames, dtype=np.uint64)
    nb = ctypes.c_uint64(0)
    c.cmp_image_ck_layout.restype = ctypes.c_uint64
    c.cmp_image_ck_layout.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p,
                                      ctypes.c_void_p, ctypes.c_void_p]
    c.cmp_image_ck_layout(fbs.ctypes.data, 2, frames, None, None, ctypes.byref(nb))
    blocks = np.zeros(2 * nb.value, dtype=np.uint32)
    total = c.cmp_image_ck_layout(fbs.ctypes.data, 2, frames, off.ctypes.data, blocks.ctypes.data, None)
    addr = (src.data_ptr() + np.arange(frames, dtype=np.uint64) * np.uint64(2 * n)).astype(np.uint64)
    d_addr, d_off = torch.from_numpy(addr.view(np.int64)).cuda(), torch.from_numpy(off.view(np.int64)).cuda()
    d_n = torch.full((frames,), n, dtype=torch.int32, device="cuda")
    d_blocks = torch.from_numpy(blocks.view(np.int32)).cuda()
    out_a = torch.zeros(frames, dtype=torch.int32, device="cuda")
    out_b = torch.zeros(frames, dtype=torch.int32, device="cuda")
    q = RaggedCk(2, frames, d_addr.data_ptr(), d_n.data_ptr(), d_off.data_ptr(), total, d_blocks.data_ptr(),
                 nb.value, out_b.data_ptr())
    c.airs_dev_checksum.restype = c.airs_dev_checksum_ragged.restype = ctypes.c_uint32
    c.airs_dev_checksum.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32,
                                    ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]
    c.airs_dev_checksum_ragged.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    calls = {"strided": lambda: c.airs_dev_checksum(dev, src.data_ptr(), 2 * n, 2, n, frames, None,
                                                     out_a.data_ptr()),
             "ragged": lambda: c.airs_dev_checksum_ragged(dev, ctypes.byref(q))}
    flush = torch.empty(512 << 20, dtype=torch.uint8, device="cuda")

    def timed(fn):
        flush.fill_(1)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        assert fn() == 0
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3  # us

    for fn in calls.values():  # warm up: code objects, the products scratch
        for _ in range(2):
            assert fn() == 0
    torch.cuda.synchronize()
    assert torch.equal(out_a, out_b), "the ragged XXH32 differs from airs_dev_checksum"
    t = {k: [] for k in calls}
    for _ in range(reps):
        for k, fn in calls.items():
            t[k].append(timed(fn))
    res = {"workload": {"frames": frames, "samples_per_frame": n, "sample_bytes": 2, "cold": True, "reps": reps,
                        "products_bytes": int(total), "product_workgroups": int(nb.value)}}
    for k in calls:
        res[k + "_us"] = {"median": statistics.median(t[k]), "min": min(t[k]), "max": max(t[k]), "all": t[k]}
    res["ragged_over_strided"] = res["ragged_us"]["median"] / res["strided_us"]["median"]
    print(json.dumps(res))
    if out_path:
        with open(out_path, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if name == "ragged":
    ragged_main(sys.argv[2] if len(sys.argv) > 2 else None)
    sys.exit(0)
wl = bench.WORKLOADS[name]
stream = torch.cuda.current_stream()
eng = lib.engine(stream.cuda_stream)
n, nf = wl["n"], wl["nctx"] * wl["fpc"]
stride = 2 * n
src = torch.empty(nf * stride, dtype=torch.uint8, device="cuda")
for j, f in enumerate(bench.frame_ids(wl, 0, 1)):
    eng.synthesize(src.data_ptr() + j * stride, 2, wl["seed"], f, n, 1, stride, bench.noise_w(wl, f))
cap = lib.compress_bound(2 * n)
cap = cap if not api.is_error(cap) else 3 * 2 * n + 64
dstride = (cap + 7) // 8 * 8
dst = torch.empty(nf * dstride, dtype=torch.uint8, device="cuda")
sizes = torch.zeros(nf, dtype=torch.int32, device="cuda")
ctxs = pkg.context_array(1)
lib.initialise(ctxs[0], api.CmpParams(**dict(wl["params"], checksum_enabled=1)))
for k in range(2):
    assert eng.compress(ctxs, nf, "u16", src.data_ptr(), stride, stride, dst.data_ptr(), dstride, cap,
                        sizes.data_ptr()) == 0
torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record(stream)
for k in range(5):
    assert eng.compress(ctxs, nf, "u16", src.data_ptr(), stride, stride, dst.data_ptr(), dstride, cap,
                        sizes.data_ptr()) == 0
e1.record(stream)
torch.cuda.synchronize()
ms = e0.elapsed_time(e1) / 5
print(json.dumps(dict(workload=name, checksum=True, ms_per_call=round(ms, 4),
                      GBps=round(nf * 2 * n / (ms * 1e-3) / 1e9, 1))))
