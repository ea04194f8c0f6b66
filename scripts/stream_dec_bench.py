#!/usr/bin/env python3
"""Payload-only stream decode: the cfg2s stream -- 64 Mi u16
samples, DIFF + GOLOMB_ZERO g = 32, ONE bit stream from cmp_gpu_encode_stream,
left on the device -- decoded by cmp_gpu_decode_stream, alternating in one
process with cmp_gpu_decompress over the same samples as cfg2's 16 frames (the
yardstick).  Both outputs are checked against the input.  Times are the wall
clock of the call up to a device synchronise (the parse's host
synchronisations included): medians of the repeats after 2 warm-ups, and the
frame form's relative spread (max - min over median).
usage: stream_dec_bench.py [--repeats R] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=21, help="at least 9")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_decode_cfg2s.json"))
args = ap.parse_args()
repeats = max(args.repeats, 9)

pkg = bench.load_pkg()
api = pkg.cmpapi
lib = pkg.load()
wl = bench.WORKLOADS["cfg2s"]
prm = wl["params"]
pre, enc, g = prm["primary_preprocessing"], prm["primary_encoder_type"], prm["primary_encoder_param"]
stream = torch.cuda.current_stream()
eng = lib.engine(stream.cuda_stream)
n, nf = wl["n"], wl["nctx"] * wl["fpc"]
N = n * nf
stride = 2 * n
src = torch.empty(nf * stride, dtype=torch.uint8, device="cuda")
for j, f in enumerate(bench.frame_ids(wl, 0, 1)):
    eng.synthesize(src.data_ptr() + j * stride, 2, wl["seed"], f, n, 1, stride, wl["W"])

# the stream (stays on the device; the bytes after it are not zero)
scap = 6 * N + 64
sbuf = torch.full((scap + 64,), 0xAB, dtype=torch.uint8, device="cuda")
ssize = torch.zeros(1, dtype=torch.int32, device="cuda")
r = eng.encode_stream("u16", src.data_ptr(), N, pre, enc, g, 0, sbuf.data_ptr(), scap, ssize.data_ptr())
assert r == 0, api.error_name(r)
assert eng.synchronize() == 0
size = int(ssize.cpu().numpy().astype(np.uint32)[0])
assert not api.is_error(size), api.error_name(size)

# the same samples as cfg2's 16 frames
cap = lib.compress_bound(2 * n)
cap = cap if not api.is_error(cap) else 3 * 2 * n + 64
cap = (cap + 7) // 8 * 8
fbuf = torch.empty(nf * cap, dtype=torch.uint8, device="cuda")
fsizes = torch.zeros(nf, dtype=torch.int32, device="cuda")
ctxs = pkg.context_array(1)
assert not api.is_error(lib.initialise(ctxs[0], api.CmpParams(**prm)))
assert eng.compress(ctxs, nf, "u16", src.data_ptr(), stride, stride, fbuf.data_ptr(), cap, cap,
                    fsizes.data_ptr()) == 0
assert eng.synchronize() == 0

out_s = torch.zeros(N, dtype=torch.int16, device="cuda")
out_f = torch.zeros(N, dtype=torch.int16, device="cuda")
st_s = torch.zeros(1, dtype=torch.int32, device="cuda")
st_f = torch.zeros(nf, dtype=torch.int32, device="cuda")


def dec_stream():
    r = eng.decode_stream(sbuf.data_ptr(), size, N, pre, enc, g, 0, out_s.data_ptr(), st_s.data_ptr())
    assert r == 0, api.error_name(r)


def dec_frames():
    assert eng.decompress(fbuf.data_ptr(), cap, cap, nf, out_f.data_ptr(), 2 * n, n, st_f.data_ptr()) == 0


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


for _ in range(2):
    timed(dec_stream)
    timed(dec_frames)
t_s, t_f = [], []
for _ in range(repeats):
    t_s.append(timed(dec_stream))
    t_f.append(timed(dec_frames))
ok_s = int(st_s.cpu().numpy().astype(np.uint32)[0]) == N and torch.equal(out_s.view(torch.uint8), src)
ok_f = bool((st_f.cpu().numpy() == n).all()) and torch.equal(out_f.view(torch.uint8), src)
med_s, med_f = float(np.median(t_s)), float(np.median(t_f))
res = dict(workload="cfg2s", samples=N, stream_bytes=size, frames=nf, samples_per_frame=n, repeats=repeats,
           t_stream_ms=round(med_s, 3), t_frames_ms=round(med_f, 3),
           t_stream_all_ms=[round(t, 3) for t in t_s], t_frames_all_ms=[round(t, 3) for t in t_f],
           frames_rel_spread=round((max(t_f) - min(t_f)) / med_f, 4),
           stream_rel_spread=round((max(t_s) - min(t_s)) / med_s, 4),
           stream_over_frames=round(med_s / med_f, 3), stream_GBps=round(2 * N / (med_s * 1e-3) / 1e9, 1),
           frames_GBps=round(2 * N / (med_f * 1e-3) / 1e9, 1), roundtrip_ok=bool(ok_s), frames_roundtrip_ok=bool(ok_f),
           note="wall clock of the call up to a device synchronise, host synchronisations of the parse included; "
                "medians; the two forms alternate in one process; outputs checked against the input")
print(json.dumps(res))
if not (ok_s and ok_f):
    sys.exit("round trip failed")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
eng.close()
