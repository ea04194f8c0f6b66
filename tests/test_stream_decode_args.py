"""cmp_gpu_decode_stream: the call-level refusals of include/cmp_gpu.h, in the
order the header lists them.  Validation returns before anything touches the
device, so the real library answers with no GPU present; the engine and the
pointers are never dereferenced (placeholders).  The accepted boundary values
are shown by a later refusal answering: the checks run in the table's order,
so a call with src_size == CMP_GPU_STREAM_DECODE_MAX and num_samples ==
89478485 that is refused for its preprocessing passed both size checks."""
import ctypes

import pytest

from conftest import load_pkg

pkg = load_pkg()
api = pkg.cmpapi

BASE = 1 << 20  # a 16-byte aligned placeholder address
SAMPLES_MAX = 89478485
SIZE_MAX = 536870400  # CMP_GPU_STREAM_DECODE_MAX: 2^32 - 4096 bits


def good():
    return dict(engine=True, src=BASE, src_size=4096, num_samples=1000, preprocessing=1, encoder_type=1,
                encoder_param=32, encoder_outlier=0, dst=2 * BASE, status=3 * BASE)


def call(prod, **over):
    a = dict(good(), **over)
    engine = ctypes.create_string_buffer(64)  # never read: every case fails validation
    return api.error_name(prod.lib.cmp_gpu_decode_stream(
        ctypes.addressof(engine) if a["engine"] else None, a["src"], a["src_size"], a["num_samples"],
        a["preprocessing"], a["encoder_type"], a["encoder_param"], a["encoder_outlier"], a["dst"], a["status"]))


BAD = {
    "engine NULL": (dict(engine=False), "GENERIC"),
    "status NULL": (dict(status=None), "GENERIC"),
    "src NULL": (dict(src=None), "SRC_NULL"),
    "src 4-byte aligned": (dict(src=BASE + 4), "GENERIC"),
    "src odd": (dict(src=BASE + 1), "GENERIC"),
    "dst NULL": (dict(dst=None), "DST_NULL"),
    "dst odd": (dict(dst=2 * BASE + 1), "DST_UNALIGNED"),
    "no samples": (dict(num_samples=0), "SRC_SIZE_WRONG"),
    "one sample too many": (dict(num_samples=SAMPLES_MAX + 1), "SRC_SIZE_WRONG"),
    "2^32 - 1 samples": (dict(num_samples=0xFFFFFFFF), "SRC_SIZE_WRONG"),
    "no bytes": (dict(src_size=0), "SRC_SIZE_WRONG"),
    "one byte too many": (dict(src_size=SIZE_MAX + 1), "SRC_SIZE_WRONG"),
    "2^29 bytes": (dict(src_size=1 << 29), "SRC_SIZE_WRONG"),
    "2^32 - 1 bytes": (dict(src_size=0xFFFFFFFF), "SRC_SIZE_WRONG"),
    "IWT": (dict(preprocessing=2), "PARAMS_INVALID"),
    "MODEL": (dict(preprocessing=3), "PARAMS_INVALID"),
    "no such preprocessing": (dict(preprocessing=4), "PARAMS_INVALID"),
    "no such encoder": (dict(encoder_type=3), "PARAMS_INVALID"),
    "g = 0": (dict(encoder_param=0), "PARAMS_INVALID"),
    "g = 65536": (dict(encoder_param=65536), "PARAMS_INVALID"),
    "MULTI with outlier 0": (dict(encoder_type=2, encoder_outlier=0), "PARAMS_INVALID"),
}


@pytest.mark.parametrize("what", sorted(BAD))
def test_refused_before_the_device(prod, what):
    over, want = BAD[what]
    assert call(prod, **over) == want, what


def test_refusals_come_in_the_documented_order(prod):
    # each call breaks everything from one row of the table on: the first row answers
    rows = [("status", None, "GENERIC"), ("src", None, "SRC_NULL"), ("src", BASE + 4, "GENERIC"),
            ("dst", None, "DST_NULL"), ("dst", 2 * BASE + 1, "DST_UNALIGNED"), ("num_samples", 0, "SRC_SIZE_WRONG"),
            ("src_size", 0, "SRC_SIZE_WRONG"), ("preprocessing", 2, "PARAMS_INVALID"),
            ("encoder_param", 0, "PARAMS_INVALID")]
    for i, (_, _, want) in enumerate(rows):
        over = {}
        for k, v, _ in reversed(rows[i:]):  # an earlier row's value for a key wins
            over[k] = v
        assert call(prod, **over) == want, rows[i]


def test_boundary_values_pass_the_size_checks(prod):
    # the largest accepted sizes get past their checks: the refusal after them answers
    assert call(prod, src_size=SIZE_MAX, num_samples=SAMPLES_MAX, preprocessing=2) == "PARAMS_INVALID"
    assert call(prod, src_size=SIZE_MAX, num_samples=SAMPLES_MAX, encoder_param=0) == "PARAMS_INVALID"
    # one more of either and the size check answers first
    assert call(prod, src_size=SIZE_MAX + 1, num_samples=SAMPLES_MAX, preprocessing=2) == "SRC_SIZE_WRONG"
    assert call(prod, src_size=SIZE_MAX, num_samples=SAMPLES_MAX + 1, preprocessing=2) == "SRC_SIZE_WRONG"
    assert call(prod, src_size=1, num_samples=1, preprocessing=2) == "PARAMS_INVALID"


def test_the_limit_is_what_the_header_says():
    import os
    import re
    from conftest import ROOT
    with open(os.path.join(ROOT, "include", "cmp_gpu.h")) as f:
        m = re.search(r"#define CMP_GPU_STREAM_DECODE_MAX (\d+)u", f.read())
    # 2^32 - 4096 bits: every stream of up to 89478400 samples (48 bits each at most) fits
    assert int(m.group(1)) == pkg.STREAM_DECODE_MAX == SIZE_MAX == (2 ** 32 - 4096) // 8 == 89478400 * 6
