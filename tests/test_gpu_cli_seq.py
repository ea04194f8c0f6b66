"""airspace -d over a MODEL sequence: the whole .air file goes to the GPU as one
sequence (cmp_gpu_decompress_sequences), the model rebuilt on the device, and
every frame's checksum is verified against the decoded samples."""
import os
import subprocess

import numpy as np
import pytest

from conftest import PKG_DIR, load_pkg

pytestmark = pytest.mark.gpu
CLI = os.path.join(PKG_DIR, "bin", "airspace")
api = load_pkg().cmpapi
PARAMS = ("primary_preprocessing=DIFF,primary_encoder_type=GOLOMB_ZERO,primary_encoder_param=16,"
          "secondary_iterations=4,secondary_preprocessing=MODEL,secondary_encoder_type=GOLOMB_MULTI,"
          "secondary_encoder_param=8,secondary_encoder_outlier=107,model_rate=11,checksum_enabled=1")
NFILES, N = 12, 3001


def run(args, cwd):
    return subprocess.run([CLI] + [str(a) for a in args], capture_output=True, cwd=cwd, timeout=120)


@pytest.fixture(scope="module")
def sequence(tmp_path_factory, prod):
    """12 files of one size compressed by the CLI into one .air file."""
    if not prod.gpu_available():
        pytest.fail("GPU test run without a usable HIP device")
    d = tmp_path_factory.mktemp("seq")
    rng = np.random.default_rng(12)
    base = np.cumsum(rng.integers(-20, 21, N)) + 40000  # both halves of the u16 range
    paths, want = [], b""
    for i in range(NFILES):
        x = ((base + rng.integers(-30, 31, N) + 40 * i) & 0xFFFF).astype(np.uint16)
        p = d / f"acq{i:02d}.dat"
        p.write_bytes(x.astype(">u2").tobytes())
        paths.append(p)
        want += x.astype(">u2").tobytes()
    r = run(["-c", "--params", PARAMS] + paths + ["--stdout"], d)
    assert r.returncode == 0, r.stderr.decode()
    blob = r.stdout
    (d / "seq.air").write_bytes(blob)
    offsets, pos = [], 0
    while pos < len(blob):
        offsets.append(pos)
        pos += int.from_bytes(blob[pos + 2:pos + 5], "big")
    assert len(offsets) == NFILES
    pres = [blob[o + 15] >> 4 for o in offsets]
    assert pres == [1, 3, 3, 3, 3, 1, 3, 3, 3, 3, 1, 3]  # MODEL frames, a reset inside
    assert all((blob[o + 15] >> 3) & 1 for o in offsets)
    return d, blob, offsets, want


def test_model_sequence_roundtrips(sequence):
    d, blob, offsets, want = sequence
    r = run(["-d", "-q", d / "seq.air", "-o", d / "seq.out"], d)
    assert r.returncode == 0, r.stderr.decode()
    assert (d / "seq.out").read_bytes() == want


@pytest.mark.parametrize("frame", [0, 7])
def test_checksum_mismatch_fails_the_file(sequence, frame):
    """One checksum byte flipped (a primary frame's, a MODEL frame's): exit
    status 1 and a message naming the frame's byte offset; nothing is written."""
    d, blob, offsets, want = sequence
    end = offsets[frame + 1] if frame + 1 < len(offsets) else len(blob)
    bad = bytearray(blob)
    bad[end - 3] ^= 0x40
    name = f"bad{frame}.air"
    (d / name).write_bytes(bytes(bad))
    r = run(["-d", d / name], d)
    assert r.returncode == 1
    msg = r.stderr.decode()
    assert "checksum mismatch" in msg and f"at byte {offsets[frame]}" in msg, msg
    assert not (d / f"bad{frame}").exists()
