"""airspace -d through cmp_gpu_decompress_image: files of different sizes
compressed into one .air file (frames back to back at byte granularity, so
the frames start at odd addresses) go to the device as they are and come back
as the concatenated sample files, byte for byte; a truncated file fails with
the frame's byte offset and writes nothing."""
import os
import subprocess

import numpy as np
import pytest

import image_helpers as ih
from conftest import PKG_DIR

pytestmark = pytest.mark.gpu
CLI = os.path.join(PKG_DIR, "bin", "airspace")
PARAMS = "primary_preprocessing=DIFF,primary_encoder_type=GOLOMB_ZERO,primary_encoder_param=16,checksum_enabled=1"
SIZES = (100, 4097, 1, 20000, 333, 4097, 2048, 7)


def run(args, cwd):
    return subprocess.run([CLI] + [str(a) for a in args], capture_output=True, cwd=cwd, timeout=120)


@pytest.fixture(scope="module")
def archive(tmp_path_factory, prod):
    if not prod.gpu_available():
        pytest.fail("GPU test run without a usable HIP device")
    d = tmp_path_factory.mktemp("image")
    rng = np.random.default_rng(8)
    paths, want = [], b""
    for i, n in enumerate(SIZES):
        x = ((np.cumsum(rng.integers(-20, 21, n)) + 30000 + 900 * i) & 0xFFFF).astype(">u2")
        p = d / f"f{i}.dat"
        p.write_bytes(x.tobytes())
        paths.append(p)
        want += x.tobytes()
    r = run(["-c", "--params", PARAMS] + paths + ["--stdout"], d)
    assert r.returncode == 0, r.stderr.decode()
    blob = r.stdout
    offsets, bad = ih.walk(blob)
    assert bad is None and len(offsets) == len(SIZES)
    assert [int.from_bytes(blob[o + 5:o + 8], "big") for o in offsets] == [2 * n for n in SIZES]
    assert any(o % 2 for o in offsets), "every frame starts at an even byte"
    return d, blob, offsets, want


def test_files_of_different_sizes_roundtrip(archive):
    d, blob, offsets, want = archive
    (d / "all.air").write_bytes(blob)
    r = run(["-d", "-q", d / "all.air", "-o", d / "all.out"], d)
    assert r.returncode == 0, r.stderr.decode()
    assert (d / "all.out").read_bytes() == want


@pytest.mark.parametrize("cut", [7, 1])
def test_truncated_file_names_the_frame_and_writes_nothing(archive, cut):
    d, blob, offsets, want = archive
    name = f"cut{cut}.air"
    (d / name).write_bytes(blob[:-cut])
    r = run(["-d", d / name], d)
    assert r.returncode == 1
    msg = r.stderr.decode()
    assert f"not a valid AIRSPACE frame at byte {offsets[-1]}" in msg, msg
    assert not (d / f"cut{cut}").exists()
