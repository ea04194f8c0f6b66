"""bench.py's command line: a plain run times its steps and prints the
result line; --dump-outputs writes what the last timed step computed, the
same from run to run; --full adds the checks and side measurements after it.
dump_outputs itself is checked on host tensors (no device)."""
import importlib.util
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DUMPS = ("frame_sizes", "frame_sums", "frame_bytes")


def load_bench():
    spec = importlib.util.spec_from_file_location("airs_bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def fake_set(sizes, stride, seed=1):
    rng = np.random.default_rng(seed)
    dst = rng.integers(0, 256, len(sizes) * stride).astype(np.uint8)
    return types.SimpleNamespace(dstride=stride, dst=torch.from_numpy(dst),
                                 sizes=torch.tensor(sizes, dtype=torch.int32)), dst


def test_dump_outputs_whole_and_sampled(tmp_path, pkg):
    bench = load_bench()
    sizes = [3, 16, 1, 7, 12]
    bs, dst = fake_set(sizes, 16)
    sz = bench.frame_sizes(pkg.cmpapi, {}, bs)
    assert sz.dtype == np.uint32 and list(sz) == sizes
    frames = [dst[j * 16:j * 16 + s] for j, s in enumerate(sizes)]
    packed = np.concatenate(frames)

    bench.dump_outputs(str(tmp_path / "whole"), {}, bs, sz, 0, 1)
    got = {n: np.load(tmp_path / "whole" / f"{n}.npy") for n in DUMPS}
    assert got["frame_sizes"].dtype == np.float64 and list(got["frame_sizes"]) == sizes
    assert got["frame_sums"].dtype == np.float64 and list(got["frame_sums"]) == [int(f.sum()) for f in frames]
    assert got["frame_bytes"].dtype == np.float32 and np.array_equal(got["frame_bytes"], packed)

    # more bytes than the limit: a sample of that many, the same every time, drawn from the frames' own bytes
    bench.DUMP_MAX_BYTES = 10
    for d in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / d), {}, bs, sz, 0, 1)
    s1, s2 = (np.load(tmp_path / d / "frame_bytes.npy") for d in ("s1", "s2"))
    assert s1.shape == (10,) and np.array_equal(s1, s2)
    idx = np.sort(np.random.default_rng(bench.DUMP_SEED).integers(0, packed.size, 10))
    assert np.array_equal(s1, packed[idx])
    # several ranks share the limit and name their files
    bench.dump_outputs(str(tmp_path / "r"), {}, bs, sz, 1, 2)
    assert np.load(tmp_path / "r" / "frame_bytes_rank1.npy").shape == (5,)


def test_frame_sizes_raises_on_a_frame_error(pkg):
    bench = load_bench()
    bs, _ = fake_set([5, -30, 7], 8)
    with pytest.raises(RuntimeError, match="frame errors"):
        bench.frame_sizes(pkg.cmpapi, {}, bs)


def run_bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "cfg4", *args],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    d = tmp_path_factory.mktemp("plain")
    return run_bench("--steps", "3", "--warmup", "1", "--dump-outputs", str(d)), d


@pytest.mark.gpu
def test_plain_run_result_line_and_dump(plain):
    res, d = plain
    assert res["steps"] == 3 and res["warmup"] == 1 and res["full"] is False
    assert res["unit"] == "GB/s" and res["higher_is_better"] is True and res["dtype"] == "u16"
    in_bytes = 1024 * 65536 * 2
    assert res["ms_per_step"] > 0
    assert res["value"] == pytest.approx(in_bytes / (res["ms_per_step"] * 1e-3) / 1e9, rel=1e-3)
    # nothing beside the headline figure was run
    for k in ("bitexact_vs_reference", "cpu_baseline", "warm", "scaling_reference", "gather"):
        assert k not in res
    assert "launch_us" not in res["roofline"]
    assert sorted(os.listdir(d)) == sorted(n + ".npy" for n in DUMPS)
    a = {n: np.load(d / f"{n}.npy") for n in DUMPS}
    assert sum(os.path.getsize(d / f"{n}.npy") for n in DUMPS) <= 64_000_000
    assert a["frame_sizes"].shape == a["frame_sums"].shape == (1024,)
    assert res["config"]["compression_ratio"] == round(a["frame_sizes"].sum() / in_bytes, 4)
    assert a["frame_bytes"].dtype == np.float32 and a["frame_bytes"].size == min(int(a["frame_sizes"].sum()), 8 << 20)
    assert a["frame_bytes"].min() >= 0 and a["frame_bytes"].max() <= 255


@pytest.mark.gpu
def test_full_run_checks_and_dumps_the_same(plain, tmp_path):
    res = run_bench("--steps", "3", "--warmup", "1", "--full", "--no-cpu-baseline", "--dump-outputs", str(tmp_path))
    assert res["full"] is True and res["steps"] == 3
    assert res["bitexact_vs_reference"] is True
    assert res["roofline"]["launch_us"]["n"] == 20 and res["warm"]["value"] > 0
    for n in DUMPS:
        assert np.array_equal(np.load(tmp_path / f"{n}.npy"), np.load(plain[1] / f"{n}.npy")), n
