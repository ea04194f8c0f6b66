#!/usr/bin/env python3
"""Cost of decoding a file image (cmp_gpu_decompress_image: unpack + decode +
emit) against the strided decoder (cmp_gpu_decompress_sequences) on the same
frames pre-staged in rows, and of `airspace -d` on the file form against
another build's binary.

Workload: FRAMES frames of N u16 samples of the counter-hash signal, DIFF +
GOLOMB_ZERO g = 32, compressed on the device.  Both decoders run cold (a
buffer larger than the Infinity Cache is rewritten before every call),
interleaved, and the median of the HIP-event times is reported.  Kernel times
come from a profiler run of this script with --once image|strided.

    python scripts/image_decode_bench.py --out profiles/image_decode.json [--other-cli PATH]
"""
import argparse
import importlib.util
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "airs-compression_amd")
FRAMES, N, G = 1024, 65536, 32


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
    ap.add_argument("--other-cli", help="airspace binary of the build to compare the wall time with")
    ap.add_argument("--once", choices=["image", "strided"], help="warm up, then one cold call (for a profiler)")
    a = ap.parse_args()
    import torch
    pkg = load_pkg()
    api = pkg.cmpapi
    lib = pkg.load()
    assert lib.gpu_available(), "no HIP device"
    eng = lib.engine()

    # the frames, strided as cmp_gpu_compress leaves them
    src = torch.empty(FRAMES * N, dtype=torch.int16, device="cuda")
    assert eng.synthesize(src.data_ptr(), 2, 0xA1A5, 0, N, FRAMES, 2 * N, 32) == 0
    cap = lib.compress_bound(2 * N)
    stride = (cap + 7) // 8 * 8
    rows = torch.zeros(FRAMES * stride, dtype=torch.uint8, device="cuda")
    sizes = torch.zeros(FRAMES, dtype=torch.int32, device="cuda")
    ctxs = pkg.context_array(1)
    prm = api.CmpParams(primary_preprocessing=1, primary_encoder_type=1, primary_encoder_param=G)
    assert not api.is_error(lib.initialise(ctxs[0], prm))
    assert eng.compress(ctxs, FRAMES, "u16", src.data_ptr(), 2 * N, 2 * N, rows.data_ptr(), stride, cap,
                        sizes.data_ptr()) == 0
    assert eng.synchronize() == 0
    sz = sizes.cpu().numpy().astype(np.int64)
    assert (sz > 0).all() and (sz <= cap).all()
    # rows as narrow as the largest frame, and the file form: back to back at byte granularity
    rcap = (int(sz.max()) + 7) // 8 * 8
    host = rows.cpu().numpy().reshape(FRAMES, stride)
    staged = torch.from_numpy(np.ascontiguousarray(host[:, :rcap]).reshape(-1)).cuda()
    blob = b"".join(host[f, :sz[f]].tobytes() for f in range(FRAMES))
    offs = np.concatenate([[0], np.cumsum(sz)])[:-1].astype(np.uint64)
    image = torch.from_numpy(np.frombuffer(b"\xA5" + blob, dtype=np.uint8).copy()).cuda()  # an odd address
    del rows, host

    st = torch.zeros(FRAMES, dtype=torch.int32, device="cuda")
    out_rows = torch.zeros(FRAMES * N, dtype=torch.int16, device="cuda")
    out_img = torch.zeros(FRAMES * N, dtype=torch.int16, device="cuda")
    flush = torch.empty(512 << 20, dtype=torch.uint8, device="cuda")

    def strided():
        assert eng.decompress_sequences("u16", staged.data_ptr(), rcap, rcap, 1, FRAMES, out_rows.data_ptr(), 2 * N,
                                        N, st.data_ptr()) == 0

    def imagecall():
        rc, _ = eng.decompress_image("u16", image.data_ptr() + 1, len(blob), offs, out_img.data_ptr(),
                                     2 * N * FRAMES, st.data_ptr())
        assert rc == 0, api.error_name(rc)

    def timed(fn):
        flush.fill_(1)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        assert (st == N).all()
        return e0.elapsed_time(e1) * 1e3  # us

    for _ in range(3):  # code objects, scratch
        strided()
        imagecall()
    torch.cuda.synchronize()
    assert torch.equal(out_rows, out_img) and torch.equal(out_img, src), "the decoders disagree"
    if a.once:
        timed(imagecall if a.once == "image" else strided)
        return
    ts, ti = [], []
    for _ in range(a.reps):
        ts.append(timed(strided))
        ti.append(timed(imagecall))
    res = {
        "workload": {"frames": FRAMES, "samples_per_frame": N, "preprocessing": "DIFF", "encoder": "GOLOMB_ZERO",
                     "g": G, "compressed_bytes": int(sz.sum()), "decoded_bytes": 2 * N * FRAMES,
                     "staged_row_bytes": rcap, "cold": True, "reps": a.reps},
        "strided_us": {"median": statistics.median(ts), "min": min(ts), "max": max(ts), "all": ts},
        "image_us": {"median": statistics.median(ti), "min": min(ti), "max": max(ti), "all": ti},
    }
    res["image_over_strided"] = res["image_us"]["median"] / res["strided_us"]["median"]

    # wall time of airspace -d on the file form, this build against the other one, alternating
    clis = {"this": os.path.join(PKG_DIR, "bin", "airspace")}
    if a.other_cli:
        clis["other"] = a.other_cli
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "w.air")
        with open(path, "wb") as f:
            f.write(blob)
        want = src.cpu().numpy().astype(">u2").tobytes()
        wall = {k: [] for k in clis}
        for rep in range(5):
            for k, cli in clis.items():
                outp = os.path.join(d, f"{k}{rep}.out")
                t0 = time.perf_counter()
                r = subprocess.run([cli, "-d", "-q", path, "-o", outp], capture_output=True, timeout=300)
                wall[k].append(time.perf_counter() - t0)
                assert r.returncode == 0, r.stderr.decode()
                with open(outp, "rb") as f:
                    assert f.read() == want, k
                os.remove(outp)
    res["cli_wall_s"] = {k: {"median": statistics.median(v), "all": v} for k, v in wall.items()}
    if "other" in wall:
        res["cli_this_over_other"] = res["cli_wall_s"]["this"]["median"] / res["cli_wall_s"]["other"]["median"]
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
