"""airspace -c over files of mixed sizes: the files of a batch go to the GPU as
they are (big-endian, back to back) and are ONE cmp_gpu_compress_image call;
every FILE.air is a slice of the packed image.  The outputs are byte for byte
the frames of the CPU oracle's per-file loop over one context (header
identifiers excepted: they come from the clock), and airspace -d gives the
inputs back."""
import os
import subprocess

import numpy as np
import pytest

from conftest import PKG_DIR, load_pkg

pytestmark = pytest.mark.gpu
CLI = os.path.join(PKG_DIR, "bin", "airspace")
api = load_pkg().cmpapi
MODEL = dict(primary_preprocessing=1, primary_encoder_type=1, primary_encoder_param=16, secondary_iterations=2,
             secondary_preprocessing=3, secondary_encoder_type=2, secondary_encoder_param=8,
             secondary_encoder_outlier=107, model_rate=11, checksum_enabled=1)
MODEL_ARG = ("primary_preprocessing=DIFF,primary_encoder_type=GOLOMB_ZERO,primary_encoder_param=16,"
             "secondary_iterations=2,secondary_preprocessing=MODEL,secondary_encoder_type=GOLOMB_MULTI,"
             "secondary_encoder_param=8,secondary_encoder_outlier=107,model_rate=11,checksum_enabled=1")


def run(args, cwd):
    return subprocess.run([CLI] + [str(a) for a in args], capture_output=True, cwd=cwd, timeout=120)


def masked(frame):
    return frame[:8] + b"\0" * 6 + frame[14:]  # identifier bytes 8-13 come from the clock


def write_files(d, ns, seed):
    rng = np.random.default_rng(seed)
    base = np.cumsum(rng.integers(-20, 21, max(ns))) + 40000
    paths, xs = [], []
    for i, n in enumerate(ns):
        x = ((base[:n] + rng.integers(-30, 31, n) + 40 * i) & 0xFFFF).astype(np.uint16)
        p = d / f"acq{i:02d}.dat"
        p.write_bytes(x.astype(">u2").tobytes())
        paths.append(p)
        xs.append(x)
    return paths, xs


def oracle_loop(orc, par, xs):
    """One context over the files in order: the frame, or the error value."""
    ctx = api.CmpContext()
    wbs = orc.cal_work_buf_size(par, 2 * len(xs[0]))  # the CLI sizes the work buffer from the first file
    wb = api.aligned_empty(max(wbs, 2), fill=0)
    assert not api.is_error(orc.initialise(ctx, par, wb if wbs else None, wbs))
    out = []
    for x in xs:
        cap = orc.compress_bound(2 * len(x))
        dst = api.aligned_empty(cap)
        r = orc.compress_u16(ctx, dst, cap, x)
        out.append(r & 0xFFFFFFFF if api.is_error(r) else bytes(dst[:r]))
    return out


@pytest.fixture(scope="module")
def gpu(prod):
    if not prod.gpu_available():
        pytest.fail("GPU test run without a usable HIP device")


@pytest.mark.parametrize("which", ["default", "model"])
def test_mixed_sizes_match_the_per_file_loop_and_come_back(tmp_path, gpu, orc, which):
    """Default parameters: a run, a singleton, a run.  MODEL parameters with a
    pass cycle of three frames: runs of three, so that every size change meets
    a primary pass (the reference refuses it anywhere else, see below)."""
    ns = [3001] * 4 + [1234] + [3001] * 3 if which == "default" else [3001] * 3 + [1234] * 3 + [3001] * 3
    paths, xs = write_files(tmp_path, ns, 7)
    args = ["-c", "-q"] + (["--params", MODEL_ARG] if which == "model" else []) + paths
    r = run(args, tmp_path)
    assert r.returncode == 0, r.stderr.decode()
    par = api.CmpParams(**MODEL) if which == "model" else api.CmpParams()  # the CLI's defaults: all zero
    want = oracle_loop(orc, par, xs)
    for p, w in zip(paths, want):
        got = (tmp_path / (p.name + ".air")).read_bytes()
        assert masked(got) == masked(w), p.name
    if which == "model":
        assert [w[15] >> 4 for w in want] == [1, 3, 3] * 3
    # the outputs back to back are one .air file (one context, as a MODEL frame needs the frames before it)
    (tmp_path / "all.air").write_bytes(b"".join((tmp_path / (p.name + ".air")).read_bytes() for p in paths))
    r = run(["-d", "-q", tmp_path / "all.air", "-o", tmp_path / "all.out"], tmp_path)
    assert r.returncode == 0, r.stderr.decode()
    assert (tmp_path / "all.out").read_bytes() == b"".join(x.astype(">u2").tobytes() for x in xs)


def test_a_size_change_in_a_model_pass_fails_that_file(tmp_path, gpu, orc):
    """A run, a singleton, a run under MODEL parameters: the singleton meets a
    secondary pass.  As in the per-file loop the files before it are written,
    the file is named with CMP_ERR_SRC_SIZE_MISMATCH, nothing after it is
    written and the exit status is 1."""
    ns = [3001] * 4 + [1234] + [3001] * 3
    paths, xs = write_files(tmp_path, ns, 8)
    r = run(["-c", "--params", MODEL_ARG] + paths, tmp_path)
    want = oracle_loop(orc, api.CmpParams(**MODEL), xs)
    assert api.error_name(want[4]) == "SRC_SIZE_MISMATCH"
    assert r.returncode == 1
    msg = r.stderr.decode()
    assert "Compression failed for" in msg and "acq04.dat" in msg and "not allowed until reset" in msg, msg
    for p, w in zip(paths[:4], want):
        assert masked((tmp_path / (p.name + ".air")).read_bytes()) == masked(w), p.name
    for p in paths[4:]:
        assert not (tmp_path / (p.name + ".air")).exists(), p.name


def test_a_file_too_large_for_the_bound_keeps_the_reference_route(tmp_path, gpu, orc):
    """More than 5.59 MB of samples: cmp_compress_bound is an error value, the
    reference warns and goes on with the largest capacity a header describes
    (file.c:424-430).  Such a file is a batch of its own between the image
    calls of its neighbours; one context runs through all three."""
    n_big = 2_900_000
    assert api.is_error(orc.compress_bound(2 * n_big))
    ns = [3001, n_big, 3001]
    paths, xs = write_files(tmp_path, ns, 9)
    args = "primary_preprocessing=DIFF,primary_encoder_type=GOLOMB_ZERO,primary_encoder_param=32,checksum_enabled=1"
    r = run(["-c", "--params", args] + paths, tmp_path)
    assert r.returncode == 0, r.stderr.decode()
    assert r.stderr.decode().count("use maximum size") == 1
    par = api.CmpParams(primary_preprocessing=1, primary_encoder_type=1, primary_encoder_param=32, checksum_enabled=1)
    ctx = api.CmpContext()
    assert not api.is_error(orc.initialise(ctx, par))
    for p, x in zip(paths, xs):
        cap = orc.compress_bound(2 * len(x))
        cap = (1 << 24) - 1 if api.is_error(cap) else cap
        dst = api.aligned_empty(cap)
        got = orc.compress_u16(ctx, dst, cap, x)
        assert not api.is_error(got), api.error_name(got)
        assert masked((tmp_path / (p.name + ".air")).read_bytes()) == masked(bytes(dst[:got])), p.name
