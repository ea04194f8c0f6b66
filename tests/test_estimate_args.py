"""cmp_gpu_estimate: the call-level refusals of include/cmp_gpu.h, in the order
the header lists them.  Validation returns before anything touches the device,
so the real library answers with no GPU present; the engine and the pointers
are never dereferenced (placeholders), only the candidates are read.  The
accepted boundary values are shown by a later refusal answering: the checks
run in the header's order, so a call with 64 candidates, 2^20 frames and a
packed size of 2^24 - 1 that is refused for its last candidate passed every
check before the candidates."""
import ctypes

import pytest

from conftest import load_pkg

pkg = load_pkg()
api = pkg.cmpapi

BASE = 1 << 20  # a 16-byte aligned placeholder address
MAX_C, MAX_F = 64, 1 << 20
PACKED_MAX = (1 << 24) - 1  # CMP_HDR_MAX_ORIGINAL_SIZE
NONE, DIFF, IWT, MODEL = range(4)
RAW, ZERO, MULTI = range(3)
OK = (DIFF, ZERO, 32, 0)


def good():
    return dict(engine=True, batch=True, type=pkg.GPU_U16, src=BASE, src_stride=4096, src_size=4096, num_frames=3,
                model=None, model_stride=0, candidates=[OK, (NONE, MULTI, 3, 107)], num_candidates=None,
                bits=2 * BASE, best=3 * BASE, flags=0)


def call(prod, **over):
    a = dict(good(), **over)
    engine = ctypes.create_string_buffer(64)  # never read: every case fails validation
    cands = a["candidates"]
    arr = pkg.candidate_array(cands) if cands is not None else None
    nc = len(cands or ()) if a["num_candidates"] is None else a["num_candidates"]
    b = pkg.GpuEstimateBatch(type=a["type"], src=a["src"], src_stride=a["src_stride"], src_size=a["src_size"],
                             num_frames=a["num_frames"], model=a["model"], model_stride=a["model_stride"],
                             candidates=arr, num_candidates=nc, bits=a["bits"], best=a["best"], flags=a["flags"])
    return api.error_name(prod.lib.cmp_gpu_estimate(ctypes.addressof(engine) if a["engine"] else None,
                                                    ctypes.byref(b) if a["batch"] else None))


BAD = {
    "engine NULL": (dict(engine=False), "GENERIC"),
    "batch NULL": (dict(batch=False), "GENERIC"),
    "candidates NULL": (dict(candidates=None, num_candidates=2), "GENERIC"),
    "bits NULL": (dict(bits=None), "GENERIC"),
    "no frames": (dict(num_frames=0), "GENERIC"),
    "one frame too many": (dict(num_frames=MAX_F + 1), "GENERIC"),
    "no candidates": (dict(num_candidates=0), "GENERIC"),
    "one candidate too many": (dict(candidates=[OK] * (MAX_C + 1)), "GENERIC"),
    "flags": (dict(flags=1), "GENERIC"),
    "no such type": (dict(type=3), "GENERIC"),
    "bits 4-byte aligned": (dict(bits=2 * BASE + 4), "GENERIC"),
    "best 2-byte aligned": (dict(best=3 * BASE + 2), "GENERIC"),
    "src NULL": (dict(src=None), "SRC_NULL"),
    "src odd": (dict(src=BASE + 1), "GENERIC"),
    "i32 src 2-byte aligned": (dict(type=pkg.GPU_I16_IN_I32, src=BASE + 2), "GENERIC"),
    "no bytes": (dict(src_size=0), "SRC_SIZE_WRONG"),
    "odd size": (dict(src_size=4095), "SRC_SIZE_WRONG"),
    "i32 size not a multiple of 4": (dict(type=pkg.GPU_I16_IN_I32, src_size=4094), "SRC_SIZE_WRONG"),
    "packed size 2^24": (dict(src_size=PACKED_MAX + 1, src_stride=1 << 25), "HDR_ORIGINAL_TOO_LARGE"),
    "i32 packed size 2^24": (dict(type=pkg.GPU_I16_IN_I32, src_size=2 * (PACKED_MAX + 1), src_stride=1 << 26),
                             "HDR_ORIGINAL_TOO_LARGE"),
    "stride below size": (dict(src_stride=4094), "GENERIC"),
    "odd stride": (dict(src_stride=4097), "GENERIC"),
    "i32 stride not a multiple of 4": (dict(type=pkg.GPU_I16_IN_I32, src_stride=4098), "GENERIC"),
    "no such preprocessing": (dict(candidates=[OK, (4, ZERO, 32, 0)]), "PARAMS_INVALID"),
    "no such encoder": (dict(candidates=[OK, (NONE, 3, 32, 0)]), "PARAMS_INVALID"),
    "g = 0": (dict(candidates=[(NONE, ZERO, 0, 0)]), "PARAMS_INVALID"),
    "g = 65536": (dict(candidates=[OK, OK, (DIFF, MULTI, 65536, 5)]), "PARAMS_INVALID"),
    "MULTI with outlier 0": (dict(candidates=[(IWT, MULTI, 4, 0)]), "PARAMS_INVALID"),
    "MODEL without a model": (dict(candidates=[OK, (MODEL, ZERO, 4, 0)]), "PARAMS_INVALID"),
    "MODEL with an odd model": (dict(candidates=[(MODEL, ZERO, 4, 0)], model=BASE + 1, model_stride=4096),
                                "PARAMS_INVALID"),
    "MODEL with an odd model stride": (dict(candidates=[(MODEL, ZERO, 4, 0)], model=4 * BASE, model_stride=4097),
                                       "PARAMS_INVALID"),
    "MODEL with a short model stride": (dict(candidates=[(MODEL, RAW, 0, 0)], model=4 * BASE, model_stride=4094),
                                        "PARAMS_INVALID"),
    "i32 MODEL with a short model stride": (dict(type=pkg.GPU_I16_IN_I32, candidates=[(MODEL, RAW, 0, 0)],
                                                 model=4 * BASE, model_stride=2046), "PARAMS_INVALID"),
}


@pytest.mark.parametrize("what", sorted(BAD))
def test_refused_before_the_device(prod, what):
    over, want = BAD[what]
    assert call(prod, **over) == want, what


def test_refusals_come_in_the_documented_order(prod):
    # each call breaks everything from one row of the table on: the first row answers
    rows = [("bits", None, "GENERIC"), ("num_frames", 0, "GENERIC"), ("num_candidates", 0, "GENERIC"),
            ("flags", 2, "GENERIC"), ("src", None, "SRC_NULL"), ("src", BASE + 1, "GENERIC"),
            ("src_size", 0, "SRC_SIZE_WRONG"), ("src_size", PACKED_MAX + 1, "HDR_ORIGINAL_TOO_LARGE"),
            ("src_stride", 2, "GENERIC"), ("candidates", [(MODEL, ZERO, 0, 0)], "PARAMS_INVALID")]
    for i, (_, _, want) in enumerate(rows):
        over = {}
        for k, v, _ in reversed(rows[i:]):  # an earlier row's value for a key wins
            over[k] = v
        assert call(prod, **over) == want, rows[i]


def test_candidates_are_checked_in_index_order(prod):
    # candidate 0's missing model answers before candidate 1's encoder, and its own encoder before its model
    assert call(prod, candidates=[(MODEL, ZERO, 4, 0), (NONE, 7, 4, 0)]) == "PARAMS_INVALID"
    assert call(prod, candidates=[(5, ZERO, 0, 0)]) == "PARAMS_INVALID"
    # one frame needs no stride, for the samples or the models: the next refusal answers
    assert call(prod, num_frames=1, src_stride=0, model=4 * BASE, model_stride=0,
                candidates=[(MODEL, ZERO, 4, 0), (NONE, ZERO, 0, 0)]) == "PARAMS_INVALID"
    assert call(prod, num_frames=1, src_stride=1, candidates=[(NONE, ZERO, 0, 0)]) == "PARAMS_INVALID"


def test_boundary_values_pass_their_checks(prod):
    # 64 candidates, 2^20 frames and the largest packed size within 2^24 - 1 (sizes are even:
    # 2^24 - 2) get past their checks: the last candidate's refusal answers
    most = dict(num_frames=MAX_F, candidates=[OK] * (MAX_C - 1) + [(NONE, ZERO, 0, 0)], src_size=PACKED_MAX - 1,
                src_stride=PACKED_MAX - 1)
    assert call(prod, **most) == "PARAMS_INVALID"
    assert call(prod, **dict(most, type=pkg.GPU_I16_IN_I32, src_size=2 * (PACKED_MAX - 1),
                             src_stride=2 * (PACKED_MAX - 1))) == "PARAMS_INVALID"
    # one more of any and its own check answers first
    assert call(prod, **dict(most, num_frames=MAX_F + 1)) == "GENERIC"
    assert call(prod, **dict(most, candidates=[OK] * MAX_C + [(NONE, ZERO, 0, 0)])) == "GENERIC"
    assert call(prod, **dict(most, src_size=PACKED_MAX + 1, src_stride=1 << 25)) == "HDR_ORIGINAL_TOO_LARGE"


def test_the_limits_are_what_the_header_says():
    import os
    import re
    from conftest import ROOT
    with open(os.path.join(ROOT, "include", "cmp_gpu.h")) as f:
        text = f.read()
    assert int(re.search(r"#define CMP_GPU_ESTIMATE_MAX_CANDIDATES (\d+)u", text).group(1)) == MAX_C \
        == pkg.ESTIMATE_MAX_CANDIDATES
    assert int(re.search(r"#define CMP_GPU_ESTIMATE_MAX_FRAMES (\d+)u", text).group(1)) == MAX_F \
        == pkg.ESTIMATE_MAX_FRAMES
