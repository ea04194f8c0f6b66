"""The device checksum's three entry points (checksum.hip: airs_dev_checksum,
airs_dev_checksum_n, airs_dev_checksum_ragged) called directly on the same
samples and compared with the oracle's orc_checksum_u16.  They share one XXH32
body and differ in geometry, so each must give the oracle's value for every
frame size at which the body takes another path: no stripe (under 8 samples),
tails of every length, one and several round quads (32 samples), the
look-ahead batch of 128 rounds (1024 samples) with exactly one batch and with
its remainders.

23 frames lie in one strided buffer, 2056 samples apart: u16 on the 16-byte
grid, u16 with 6 bytes of padding in the stride (bases leave the grid: the
sample-by-sample path), and 4-byte samples with junk upper halves."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NS = [1, 2, 3, 4, 7, 8, 9, 15, 16, 17, 31, 32, 33, 1016, 1023, 1024, 1025, 1031, 1032, 1033, 2047, 2048, 2056]
NF, STRIDE_SAMPLES = len(NS), 2056
SENTINEL = 0x5EC7E1A5
FORMS = {"u16": (2, 0), "u16-pad6": (2, 6), "i16-in-i32-junk": (4, 0)}  # sample bytes, stride padding


class RaggedCk(ctypes.Structure):  # struct airs_ragged_ck (csrc/airs_dev.h)
    _fields_ = [("sample_bytes", ctypes.c_uint32), ("frames", ctypes.c_uint32), ("src", ctypes.c_void_p),
                ("n", ctypes.c_void_p), ("off", ctypes.c_void_p), ("bytes", ctypes.c_uint64),
                ("blocks", ctypes.c_void_p), ("num_blocks", ctypes.c_uint32), ("out", ctypes.c_void_p)]


@pytest.fixture(scope="module")
def dev(prod):
    """The library's C entry points, an engine and its airs_dev_engine."""
    if not prod.gpu_available():
        pytest.fail("GPU test run without a usable HIP device")
    c = prod.lib
    c.airs_dev_checksum.restype = c.airs_dev_checksum_n.restype = c.airs_dev_checksum_ragged.restype = ctypes.c_uint32
    c.airs_dev_checksum.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32,
                                    ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]
    c.airs_dev_checksum_n.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32,
                                      ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]
    c.airs_dev_checksum_ragged.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    c.cmp_image_ck_layout.restype = ctypes.c_uint64
    c.cmp_image_ck_layout.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p,
                                      ctypes.c_void_p, ctypes.c_void_p]
    eng = prod.engine(torch.cuda.current_stream().cuda_stream)  # the tensors' stream
    # struct cmp_gpu_engine (csrc/cmp_engine.h) begins with its airs_dev_engine pointer
    handle = eng.handle if isinstance(eng.handle, int) else eng.handle.value
    yield c, eng, ctypes.c_void_p.from_address(handle).value
    eng.close()


class Samples:
    """One form's frames on the device and the oracle's checksum of the first
    n samples of every frame, computed once per n."""

    def __init__(self, orc_ext, form):
        self.sb, pad = FORMS[form]
        self.stride = STRIDE_SAMPLES * self.sb + pad
        rng = np.random.default_rng(419 + pad + self.sb)
        self.x = rng.integers(0, 1 << 16, (NF, STRIDE_SAMPLES)).astype(np.uint16)
        if self.sb == 4:
            stored = self.x.astype(np.uint32) | (rng.integers(0, 1 << 16, self.x.shape).astype(np.uint32) << 16)
        else:
            stored = self.x
        buf = np.zeros(NF * self.stride, dtype=np.uint8)
        for f in range(NF):
            buf[f * self.stride:f * self.stride + STRIDE_SAMPLES * self.sb] = stored[f].view(np.uint8)
        self.src = torch.from_numpy(buf).cuda()
        self.orc_ext, self.known = orc_ext, {}

    def want(self, f, n):
        if (f, n) not in self.known:
            v = np.ascontiguousarray(self.x[f, :n])
            self.known[f, n] = int(self.orc_ext.orc_checksum_u16(v.ctypes.data, n))
        return self.known[f, n]


@pytest.fixture(scope="module")
def samples(orc_ext):
    return {form: Samples(orc_ext, form) for form in FORMS}


def sentinels():
    return torch.full((NF,), SENTINEL, dtype=torch.int32, device="cuda")


def values(eng, out):
    assert eng.synchronize() == 0
    return [int(v) for v in out.cpu().numpy().view(np.uint32)]


def checksum_n(dev, s, frame_n):
    c, eng, e = dev
    out = sentinels()
    d_n = torch.tensor(frame_n, dtype=torch.int32, device="cuda")
    assert c.airs_dev_checksum_n(e, s.src.data_ptr(), s.stride, s.sb, max(frame_n), d_n.data_ptr(), NF,
                                 out.data_ptr()) == 0
    return values(eng, out)


@pytest.mark.parametrize("form", sorted(FORMS))
def test_checksum_n_writes_the_frames_that_have_samples(dev, samples, form):
    s = samples[form]
    frame_n = list(NS)
    frame_n[4] = frame_n[16] = 0  # a frame without a stripe and one past the look-ahead batch
    got = checksum_n(dev, s, frame_n)
    for f, n in enumerate(frame_n):
        assert got[f] == (s.want(f, n) if n else SENTINEL), (f, n, hex(got[f]))


@pytest.mark.parametrize("form", sorted(FORMS))
def test_ragged_equals_the_oracle_and_checksum_n(dev, samples, form):
    c, eng, e = dev
    s = samples[form]
    fbs = np.array([n * s.sb for n in NS], dtype=np.uint32)
    off = np.zeros(NF, dtype=np.uint64)
    nb = ctypes.c_uint64(0)
    c.cmp_image_ck_layout(fbs.ctypes.data, s.sb, NF, None, None, ctypes.byref(nb))
    blocks = np.zeros(2 * max(nb.value, 1), dtype=np.uint32)
    total = c.cmp_image_ck_layout(fbs.ctypes.data, s.sb, NF, off.ctypes.data, blocks.ctypes.data, None)
    addr = (s.src.data_ptr() + np.arange(NF, dtype=np.uint64) * np.uint64(s.stride)).astype(np.uint64)
    d_addr, d_off = torch.from_numpy(addr.view(np.int64)).cuda(), torch.from_numpy(off.view(np.int64)).cuda()
    d_n = torch.tensor(NS, dtype=torch.int32, device="cuda")
    d_blocks = torch.from_numpy(blocks.view(np.int32)).cuda()
    out = sentinels()
    q = RaggedCk(s.sb, NF, d_addr.data_ptr(), d_n.data_ptr(), d_off.data_ptr(), total, d_blocks.data_ptr(),
                 nb.value, out.data_ptr())
    assert c.airs_dev_checksum_ragged(e, ctypes.byref(q)) == 0
    got = values(eng, out)
    assert got == [s.want(f, n) for f, n in enumerate(NS)]
    assert got == checksum_n(dev, s, NS)


@pytest.mark.parametrize("n", [7, 1025])
@pytest.mark.parametrize("form", sorted(FORMS))
def test_checksum_of_equal_frames_and_of_a_frame_list(dev, samples, form, n):
    c, eng, e = dev
    s = samples[form]
    out = sentinels()
    assert c.airs_dev_checksum(e, s.src.data_ptr(), s.stride, s.sb, n, NF, None, out.data_ptr()) == 0
    assert values(eng, out) == [s.want(f, n) for f in range(NF)]
    listed = [22, 0, 17, 16, 5]
    d_list = torch.tensor(listed, dtype=torch.int32, device="cuda")
    out = sentinels()
    assert c.airs_dev_checksum(e, s.src.data_ptr(), s.stride, s.sb, n, len(listed), d_list.data_ptr(),
                               out.data_ptr()) == 0
    assert values(eng, out) == [s.want(f, n) if f in listed else SENTINEL for f in range(NF)]
