"""The Rice/ZERO frame kernel (enc_rice.hip) against the
oracle: 16-bit frames of whole 16 Ki-sample segments, NONE and DIFF,
GOLOMB_ZERO with g = 2^k for k = 0 .. 7 (the kernel's range) and 8 (past it:
encode_kernel), with and without checksums.

The data are chosen for the kernel's special steps:
  * laplace noise at the scale of g (the common case: every pair fits 32 bits
    but the escapes);
  * smooth data with single-sample outliers: each outlier gives two adjacent
    zero escapes, a pair of 2 (k + 17) bits, re-coded from the table;
  * uniform random samples: escapes everywhere, more bits than the arena
    holds, so the segment is stored chunk by chunk after its look-back;
  * constant frames (every sample the shortest code) and the extreme mapped
    value 65535.
Frames of 40 segments put the vector look-back's first round (its 16
newest granules and the tail through scalar loads) and the vector rounds
behind it to work: these batches of 5, 3 and 2 frames are no multiple of 8,
so the launch's lbmode is 0 and the all-scalar look-back (rice_lookback_s)
never runs here; test_gpu_rice_lookback.py covers it.  The launch counters
(airs_dev_launch_stats) assert which kernel ran.  Bit-exact, with the
clock-derived identifier bytes 8-13 masked (one context: frame f is its f-th
primary pass).
Reference: lib/compress/cmp.c:296-312, encoder.c:327-351,
bitstream_writer.h:124-158."""
import zlib

import numpy as np
import pytest

from conftest import load_pkg
from rice_helpers import ENCODE, LB0, Launches
from rice_helpers import frame as _frame, gpu as _gpu, mask as _mask, oracle as _oracle

pytestmark = pytest.mark.gpu
api = load_pkg().cmpapi
P = api.CmpParams
SEG = 16384


@pytest.fixture(scope="module")
def eng(prod):
    if not prod.gpu_available():
        pytest.fail("GPU test run without a usable HIP device")
    e = prod.engine()
    yield e
    e.close()


CASES = []
for k in range(0, 9):
    for pre in (0, 1):
        for data in ("laplace", "outliers", "uniform", "const", "extreme"):
            CASES.append((k, pre, data))


@pytest.mark.parametrize("k,pre,data", CASES)
def test_rice_kernel_vs_oracle(prod, eng, orc, k, pre, data):
    rng = np.random.default_rng(zlib.crc32(f"{k}/{pre}/{data}".encode()))
    kind = "u16" if (k + pre) % 2 == 0 else "i16"
    checksum = (k + len(data)) % 3 == 0
    # segments per frame: 1, 3 and 40 (the scalar look-back round), ragged batch
    shapes = [(1, 5), (3, 3), (40, 2)] if data in ("laplace", "outliers") else [(1, 3), (3, 2)]
    for spf, nf in shapes:
        n = spf * SEG
        frames = [_frame(rng, kind, n, k, data) for _ in range(nf)]
        want = _oracle(orc, kind, pre, 1 << k, frames, checksum)
        with Launches(prod) as l:
            got = _gpu(prod, eng, kind, pre, 1 << k, frames, checksum)
        # one launch: the Rice kernel (lbmode 0: 5, 3 or 2 frames) up to k = 7, encode_kernel past it
        l.only(LB0 if k <= 7 else ENCODE, 1)
        bad = [f for f in range(nf) if _mask(got[f]) != _mask(want[f])]
        assert not bad, (spf, bad, [(len(got[f]), len(want[f])) for f in bad])


def test_rice_kernel_host_api(prod, orc):
    """The host API (cmp_compress_u16 stages the frame to the device) on frames
    of whole segments, one context across calls: same frames and sequence."""
    rng = np.random.default_rng(5)
    for pre, g in ((1, 32), (0, 8), (1, 1)):
        outs = []
        for lib in (prod, orc):
            lib.set_timestamp_func(lambda: (3, 4))
            ctx = api.CmpContext()
            assert not api.is_error(lib.initialise(ctx, P(primary_preprocessing=pre, primary_encoder_type=1,
                                                          primary_encoder_param=g, checksum_enabled=1)))
            res = []
            for i in range(3):
                x = _frame(np.random.default_rng(100 + i), "u16", 2 * SEG, 5, "outliers")
                cap = lib.compress_bound(x.nbytes)
                dst = api.aligned_empty(cap)
                r = lib.compress_u16(ctx, dst, cap, x)
                res.append((r, bytes(dst[:r]) if not api.is_error(r) else None))
            lib.set_timestamp_func(None)
            outs.append(res)
        assert outs[0] == outs[1], (pre, g)
    _ = rng


def test_rice_kernel_small_capacity(prod, eng, orc):
    """A capacity below the compressed size: the hardware range check drops
    the words past it and the frame reports CMP_ERR_DST_TOO_SMALL, as the
    encode kernel does."""
    import torch
    n = 2 * SEG
    x = _frame(np.random.default_rng(9), "u16", n, 5, "laplace")
    ctxs = (api.CmpContext * 1)()
    prm = P(primary_preprocessing=1, primary_encoder_type=1, primary_encoder_param=32)
    assert not api.is_error(prod.initialise(ctxs[0], prm))
    src = torch.from_numpy(x.view(np.uint8).copy()).cuda()
    for cap in (64, 4096, 20000):
        dst = torch.zeros(cap + 64, dtype=torch.uint8, device="cuda")
        sizes = torch.zeros(1, dtype=torch.int32, device="cuda")
        r = eng.compress(ctxs, 1, "u16", src.data_ptr(), 2 * n, 2 * n, dst.data_ptr(), cap + 64, cap,
                         sizes.data_ptr(), 0)
        assert r == 0
        assert eng.synchronize() == 0
        s = int(sizes.cpu().numpy().astype(np.uint32)[0])
        assert api.is_error(s) and api.error_name(s) == "DST_TOO_SMALL", api.error_name(s)
        assert not dst[cap:].any().item()  # nothing past the capacity
