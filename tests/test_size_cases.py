"""CPU: the frames of exact size (size_cases.py) and the cases built from them
(size_limit_cases.py) before the GPU tests rely on them.

  - every case meets its self-check: the oracle returns the intended size for
    every built frame at full capacity, AUTO frames select the intended k, and
    the MODEL frames at a short capacity lose their model from the intended
    sample on;
  - the oracle equals the recorded reference (tests/golden/size_cases.json,
    made by golden/gen_size_golden.py from the compiled reference): the return
    value of every call and a digest over frame bytes, identifier, sequence
    number, model size and work buffer after every call;
  - where the reference is built, the oracle equals it live on every case.
"""
import json
import os

import numpy as np
import pytest

import size_cases as sc
import size_limit_cases as lc
from conftest import GOLDEN_DIR, load_pkg

api = load_pkg().cmpapi

with open(os.path.join(GOLDEN_DIR, "size_cases.json")) as _f:
    GOLD = json.load(_f)["cases"]

GROUPS = ("cap/rice_lb0", "cap/rice_lb1", "cap/encode", "cap/auto", "cap/raw", "fb/", "failbit/", "size24/", "fb24/")


@pytest.fixture(scope="module")
def catalogue(orc):
    return lc.cpu_catalogue(orc)


def _group(catalogue, group):
    return {k: v for k, v in catalogue.items() if k.startswith(group)}


def test_catalogue_is_the_recorded_one(catalogue):
    assert set(catalogue) == set(GOLD)
    assert all(any(k.startswith(g) for g in GROUPS) for k in catalogue)


@pytest.mark.parametrize("group", GROUPS)
def test_cases_meet_their_self_check(orc, orc_ext, catalogue, group):
    cases = _group(catalogue, group)
    assert cases
    for case in cases.values():
        lc.self_check(orc, case, orc_ext)


@pytest.mark.parametrize("group", GROUPS)
def test_oracle_equals_recorded_reference(orc, orc_ext, catalogue, group):
    bad = []
    for name, case in _group(catalogue, group).items():
        tr = lc.trace(orc, case, orc_ext)
        if [t[0] for t in tr] != GOLD[name]["returns"] or lc.trace_digest(tr) != GOLD[name]["digest"]:
            bad.append(name)
    assert not bad, bad[:10]


@pytest.mark.parametrize("group", GROUPS)
def test_oracle_equals_reference_live(orc, ref, orc_ext, catalogue, group):
    bad = [name for name, case in _group(catalogue, group).items()
           if lc.trace(orc, case, orc_ext) != lc.trace(ref, case, orc_ext)]
    assert not bad, bad[:10]


def test_capacity_cases_straddle_their_capacity(catalogue):
    """In every capacity call at least four frames are at most the capacity
    and four above it; with the checksum on, its four bytes straddle the
    capacity in four frames (the recorded reference decides which fit)."""
    for name, case in catalogue.items():
        if not name.startswith("cap/") or name.startswith("cap/raw"):
            continue
        ret = GOLD[name]["returns"]
        assert sum(not api.is_error(r) for r in ret) >= 4, name
        assert sum(r == lc.TOO_SMALL for r in ret) >= 4, name
        assert [r for r in ret if not api.is_error(r)] == [s for s in case.want.values() if s <= case.cap], name
        if case.params.checksum_enabled:
            assert sum(s - 4 <= case.cap < s for s in case.want.values()) == 4, name
    raw = {name: GOLD[name]["returns"] for name in catalogue if name.startswith("cap/raw")}
    assert sum(not api.is_error(r[0]) for r in raw.values()) >= 4
    assert sum(r[0] == lc.TOO_SMALL for r in raw.values()) >= 4


def test_fallback_cases_hold_both_outcomes_in_both_passes(orc, catalogue):
    """The oracle's output of every fallback case has raw-1 and raw compressed
    and raw+1 written raw, as the primary and as the secondary pass."""
    import batch_scenarios as bs
    for name, case in _group(catalogue, "fb/").items():
        frames, _ = bs.run_batch_host(orc, api, *case.batch())
        edges = lc.fallback_edges(case, frames)
        for sec in (0, 1):
            assert [edges[(d, sec)] for d in lc.FB_OFFS] == ["compressed"] * 3 + ["raw"] * 2, (name, sec)


def test_length_table_against_the_oracle(orc):
    """The restated code lengths, one mapped value at a time: a frame of one
    sample (NONE) has 22 + ceil(length / 8) bytes, and a frame of eight equal
    samples 22 + length bytes, for GOLOMB_ZERO and GOLOMB_MULTI at powers of
    two and other g."""
    rng = np.random.default_rng(1)
    for enc, g, outl in ((1, 1, 0), (1, 3, 0), (1, 16, 0), (1, 256, 0), (1, 1000, 0), (1, 65535, 0),
                         (2, 8, 107), (2, 5, 40), (2, 1, 24), (2, 300, 60000)):
        t = sc.length_table(enc, g, outl)
        p = api.CmpParams(primary_encoder_type=enc, primary_encoder_param=g, primary_encoder_outlier=outl)
        ms = np.unique(np.concatenate([np.arange(0, 40), rng.integers(0, 65536, 60), [65535, 32767, 32768],
                                       np.flatnonzero(np.diff(t))[:200] + 1]))
        for m in ms:
            x = sc.samples("u16", sc.NONE, np.full(8, m), rng)
            assert sc.oracle_size(orc, api, "u16", p, x)[0] == 22 + int(t[m]), (enc, g, outl, int(m))
