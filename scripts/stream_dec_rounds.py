#!/usr/bin/env python3
"""Worst case of the decoder's settle rounds on a payload-only stream (DESIGN.md
3.4.2): NONE + GOLOMB_MULTI g = 1, outlier 24 over samples of magnitude 8300 and
more, so that every codeword is 31 ones, a zero and 16 random raw bits.  Raw
bits that end in ones run into the next codeword's ones, a parse begun at a
guessed position then meets an invalid codeword, its workgroup's last exit is
the invalid sentinel, and the next workgroup parses again in the next round:
corrections travel one workgroup per host-synchronised round.  Prints the wall
clock of cmp_gpu_decode_stream up to a device synchronise against the stream's
size.  usage: stream_dec_rounds.py [WORKGROUPS ...]   (default 64 256 1024)"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402

pkg = bench.load_pkg()
api = pkg.cmpapi
lib = pkg.load()
eng = lib.engine()
for wgs in [int(a) for a in sys.argv[1:]] or [64, 256, 1024]:
    n = wgs * 16384 * 8 // 48  # 48 bits per sample, 16384 bytes of stream per workgroup
    g = torch.Generator(device="cuda").manual_seed(5)
    mag = torch.randint(8300, 32768, (n,), generator=g, device="cuda", dtype=torch.int32)
    sign = torch.randint(0, 2, (n,), generator=g, device="cuda", dtype=torch.int32) * 2 - 1
    x = (mag * sign).to(torch.int16)
    cap = 6 * n + 64
    enc = torch.full((cap + 64,), 0xAB, dtype=torch.uint8, device="cuda")
    size = torch.zeros(1, dtype=torch.int32, device="cuda")
    assert eng.encode_stream("i16", x.data_ptr(), n, 0, 2, 1, 24, enc.data_ptr(), cap, size.data_ptr()) == 0
    assert eng.synchronize() == 0
    s = int(size.cpu().numpy().astype(np.uint32)[0])
    dst = torch.zeros(n + 64, dtype=torch.int16, device="cuda")
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    for rep in range(2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = eng.decode_stream(enc.data_ptr(), s, n, 0, 2, 1, 24, dst.data_ptr(), st.data_ptr())
        assert r == 0 and eng.synchronize() == 0
        dt = time.perf_counter() - t0
        print("workgroups", (s + 16383) // 16384, "n", n, "bytes", s, "status", int(st.cpu()[0]), "equal",
              bool(torch.equal(dst[:n], x)), "decode s %.4f" % dt, flush=True)
eng.close()
