#!/usr/bin/env python3
"""Decoding whole MODEL sequences: cfg5_model's frames, written
by the GPU encoder, decoded three ways in one process:

  t_seq   cmp_gpu_decompress_sequences: one call, the models rebuilt on the chip
  t_flat  cmp_gpu_decompress over the same frames with every frame's model
          precomputed from the known inputs: decoding with no chain at all
  t_loop  one cmp_gpu_decompress per acquisition with the models rebuilt on the
          host between the calls: what a caller had to do without the first

Wall clock around each variant, ending in a device synchronise (the calls'
own host synchronisations included); t_seq and t_flat alternate; medians, and
the relative spread (max - min over median) of the t_flat repeats.  Every
variant's output is checked against the inputs' low halves.
usage: decode_seq_bench.py [--contexts N] [--repeats R] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import configs  # noqa: E402  (tests/configs.py: the BASELINE workloads)

ap = argparse.ArgumentParser()
ap.add_argument("--contexts", type=int, default=None)
ap.add_argument("--repeats", type=int, default=9)
ap.add_argument("--out", default=None)
args = ap.parse_args()

pkg = configs.load_pkg()
api = pkg.cmpapi
lib = pkg.load()
if not lib.gpu_available():
    sys.exit("decode_seq_bench.py needs the GPU")
eng = lib.engine(torch.cuda.current_stream().cuda_stream)
cfg = dict(configs.CONFIGS["cfg5_model"])
if args.contexts:
    cfg["nctx"] = args.contexts
n, nctx, fpc = cfg["n"], cfg["nctx"], cfg["fpc"]
nf = nctx * fpc
rate = cfg["params"]["model_rate"]

# inputs and frames, all on the device
sstride = 4 * n
src = torch.empty(nf * sstride, dtype=torch.uint8, device="cuda")
assert eng.synthesize(src.data_ptr(), 4, cfg["seed"], 0, n, nf, sstride, cfg["W"]) == 0
cap = lib.compress_bound(2 * n)
cap = cap if not api.is_error(cap) else 3 * 2 * n + 64
fstride = (cap + 7) // 8 * 8
frames = torch.empty(nf * fstride, dtype=torch.uint8, device="cuda")
sizes = torch.zeros(nf, dtype=torch.int32, device="cuda")
prm = api.CmpParams(**cfg["params"])
wbs = lib.cal_work_buf_size(prm, sstride)
wstride = (wbs + 15) // 16 * 16
work = torch.zeros(nctx * wstride, dtype=torch.uint8, device="cuda")
ctxs = pkg.context_array(nctx)
for c in range(nctx):
    assert not api.is_error(lib.initialise(ctxs[c], prm, work.data_ptr() + c * wstride, wbs))
torch.cuda.synchronize()
assert eng.compress(ctxs, fpc, cfg["kind"], src.data_ptr(), sstride, sstride, frames.data_ptr(), fstride, cap,
                    sizes.data_ptr()) == 0
assert eng.synchronize() == 0
sz = sizes.cpu().numpy().astype(np.uint32)
assert not any(api.is_error(int(s)) for s in sz)
fcap = (int(sz.max()) + 7) // 8 * 8  # bytes readable per frame

# the expected samples, and for t_flat the model every frame was encoded
# against (cmp.c:120-142, sign-extending: i16 in i32)
want = (((src.view(torch.int32).view(nctx, fpc, n) & 0xFFFF) ^ 0x8000) - 0x8000).to(torch.int16)
models = torch.zeros(nctx, fpc, n, dtype=torch.int16, device="cuda")
m = want[:, 0].to(torch.int32)
for a in range(1, fpc):
    models[:, a] = m.to(torch.int16)
    m = ((m * rate + want[:, a].to(torch.int32) * (16 - rate)) >> 4).to(torch.int16).to(torch.int32)
final_model = m.to(torch.int16)
del src

out = torch.zeros(nf * n, dtype=torch.int16, device="cuda")
st = torch.zeros(nf, dtype=torch.int32, device="cuda")
mod = torch.zeros(nctx * n, dtype=torch.int16, device="cuda")
mod_n = torch.zeros(nctx, dtype=torch.int32, device="cuda")


def run_seq():
    assert eng.decompress_sequences(cfg["kind"], frames.data_ptr(), fstride, fcap, nctx, fpc, out.data_ptr(), 2 * n,
                                    n, st.data_ptr(), mod.data_ptr(), 2 * n, mod_n.data_ptr()) == 0


def run_flat():
    assert eng.decompress(frames.data_ptr(), fstride, fcap, nf, out.data_ptr(), 2 * n, n, st.data_ptr(),
                          models.data_ptr(), 2 * n) == 0


host_x = np.empty((nctx, n), dtype=np.int16)
step_model = torch.zeros(nctx, n, dtype=torch.int16, device="cuda")


def run_loop():
    """Acquisition a of every context per call; the model rebuilt on the host
    from the samples read back, as a caller without the sequence call must."""
    hm = None
    for a in range(fpc):
        assert eng.decompress(frames.data_ptr() + a * fstride, fpc * fstride, fcap, nctx,
                              out.data_ptr() + a * 2 * n, fpc * 2 * n, n, st.data_ptr(),
                              step_model.data_ptr() if a else 0, 2 * n) == 0
        assert eng.synchronize() == 0
        if a + 1 == fpc:
            break
        host_x[:] = out.view(nctx, fpc, n)[:, a].cpu().numpy()
        if a == 0:
            hm = host_x.astype(np.int32)
        else:
            hm = ((hm * rate + host_x.astype(np.int32) * (16 - rate)) >> 4).astype(np.int16).astype(np.int32)
        step_model.copy_(torch.from_numpy(hm.astype(np.int16)))


def check(what):
    torch.cuda.synchronize()
    assert torch.equal(out.view(nctx, fpc, n), want), what


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


for fn, what in ((run_seq, "seq"), (run_flat, "flat")):
    for _ in range(2):
        out.zero_()
        fn()
        check(what)
        if what == "seq":
            assert bool((st.cpu().numpy() == n).all()) and bool((mod_n.cpu().numpy() == n).all())
            assert torch.equal(mod.view(nctx, n), final_model)
out.zero_()
run_loop()
check("loop")

t_seq, t_flat, t_loop = [], [], []
for _ in range(args.repeats):
    t_seq.append(timed(run_seq))
    t_flat.append(timed(run_flat))
for _ in range(3):
    t_loop.append(timed(run_loop))


def med(v):
    return float(np.median(v))


spread = (max(t_flat) - min(t_flat)) / med(t_flat)
res = dict(workload="cfg5_model", contexts=nctx, frames=nf, samples_per_frame=n, repeats=args.repeats,
           t_seq_ms=round(med(t_seq), 3), t_flat_ms=round(med(t_flat), 3), t_loop_ms=round(med(t_loop), 3),
           t_seq_all_ms=[round(v, 3) for v in t_seq], t_flat_all_ms=[round(v, 3) for v in t_flat],
           t_loop_all_ms=[round(v, 3) for v in t_loop], flat_rel_spread=round(spread, 4),
           seq_over_flat=round(med(t_seq) / med(t_flat), 4),
           seq_GBps=round(nf * 2 * n / (med(t_seq) * 1e-3) / 1e9, 1),
           note="wall clock per variant incl. its host synchronisations; medians; outputs checked")
print(json.dumps(res))
if args.out:
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
