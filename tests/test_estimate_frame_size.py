"""cmp_gpu_estimate_frame_size (host only): a frame's size from its payload
bits, against the oracle's frames.  The exact bits of a frame come from the
oracle's NONE stream over the residuals tiled 8 times
(estimate_helpers.exact_bits); the sizes must be equal."""
import numpy as np

import estimate_helpers as eh
from conftest import load_pkg
from estimate_helpers import DIFF, NONE, RAW, ZERO, MULTI

api = load_pkg().cmpapi
SIZE_MAX = (1 << 24) - 1  # CMP_HDR_MAX_COMPRESSED_SIZE


def test_frame_sizes_equal_the_oracle(prod, orc):
    rng = np.random.default_rng(20261021)
    for t in range(108):
        kind = ("u16", "i16", "i16_in_i32")[t % 3]
        pre = (NONE, DIFF)[(t // 3) % 2]
        enc = (RAW, ZERO, MULTI)[(t // 6) % 3]
        checksum = (t // 18) % 2
        n = int(rng.integers(1, 3000))
        g = int(1 << rng.integers(0, 16)) if rng.random() < 0.5 else int(rng.integers(1, 65536))
        outl = int(rng.integers(1, 500))
        lo = eh.low16(rng, n)
        x = eh.as_kind(rng, lo, kind)
        prm = api.CmpParams(primary_preprocessing=pre, primary_encoder_type=enc, primary_encoder_param=g,
                            primary_encoder_outlier=outl, checksum_enabled=checksum)
        ctx = api.CmpContext()
        assert not api.is_error(orc.initialise(ctx, prm))
        cap = 6 * n + 64
        want = orc.compress(kind, ctx, api.aligned_empty(cap), cap, x)
        assert not api.is_error(want), api.error_name(want)
        bits = eh.exact_bits(eh.residuals(lo, pre), enc, g, outl)
        assert prod.estimate_frame_size((pre, enc, g, outl), bits, checksum) == want, (t, kind, pre, enc, g, outl, n)


def test_header_of_an_uncompressed_frame(prod):
    assert prod.estimate_frame_size((NONE, RAW, 0, 0), 16 * 100, 0) == 16 + 200
    assert prod.estimate_frame_size((NONE, RAW, 0, 0), 16 * 100, 1) == 16 + 200 + 4
    assert prod.estimate_frame_size((DIFF, RAW, 0, 0), 16 * 100, 0) == 22 + 200
    assert prod.estimate_frame_size((NONE, ZERO, 4, 0), 16 * 100, 0) == 22 + 200
    assert prod.estimate_frame_size((NONE, ZERO, 4, 0), 0, 0) == 22
    assert prod.estimate_frame_size((NONE, ZERO, 4, 0), 1, 0) == 23
    assert prod.estimate_frame_size((NONE, ZERO, 4, 0), 8, 0) == 23
    assert prod.estimate_frame_size((NONE, ZERO, 4, 0), 9, 1) == 22 + 2 + 4


def test_size_limit(prod):
    for cand, hdr in (((NONE, RAW, 0, 0), 16), ((DIFF, MULTI, 9, 50), 22)):
        for checksum in (0, 1):
            room = SIZE_MAX - hdr - 4 * checksum  # payload bytes of the largest frame
            assert prod.estimate_frame_size(cand, 8 * room, checksum) == SIZE_MAX
            assert prod.estimate_frame_size(cand, 8 * room - 7, checksum) == SIZE_MAX
            assert api.error_name(prod.estimate_frame_size(cand, 8 * room + 1, checksum)) == "HDR_CMP_SIZE_TOO_LARGE"
    assert api.error_name(prod.estimate_frame_size((NONE, ZERO, 4, 0), 2 ** 64 - 1, 0)) == "HDR_CMP_SIZE_TOO_LARGE"
    assert api.error_name(prod.estimate_frame_size((NONE, ZERO, 4, 0), 2 ** 64 - 8, 1)) == "HDR_CMP_SIZE_TOO_LARGE"


def test_refusals(prod):
    assert api.error_name(prod.estimate_frame_size(None, 8, 0)) == "GENERIC"
    assert api.error_name(prod.estimate_frame_size((NONE, 3, 4, 0), 8, 0)) == "PARAMS_INVALID"
    assert api.error_name(prod.estimate_frame_size((NONE, ZERO, 0, 0), 8, 0)) == "PARAMS_INVALID"
    assert api.error_name(prod.estimate_frame_size((NONE, ZERO, 65536, 0), 8, 0)) == "PARAMS_INVALID"
    assert api.error_name(prod.estimate_frame_size((NONE, MULTI, 4, 0), 8, 0)) == "PARAMS_INVALID"
