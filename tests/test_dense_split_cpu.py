"""CPU: the bf16x3 image of a layer derived from its float32 image (iq_split_packed_weight_bf3_host, the host twin of the device
kernel that iq_pointnet_coalitions runs for fstn.fc3: the same index maps and the same three-term split in a loop) equals what
iq_pack_weight_bf3 gives for the plain weight, byte for byte - the padded k range included."""
import numpy as np
import pytest

from interpret_quality_amd import _lib, build


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return _lib.load()


def images(lib, w):
    cout, cin = w.shape
    w = np.ascontiguousarray(w, dtype=np.float32)
    packed = np.empty(lib.iq_packed_floats(cout, cin), dtype=np.float32)
    assert lib.iq_pack_weight(w.ctypes.data, packed.ctypes.data, cout, cin) == 0
    n = lib.iq_packed_bf3_elems(cout, cin)
    want = np.full(n, 0xabcd, dtype=np.uint16)
    got = np.full(n, 0x1234, dtype=np.uint16)
    assert lib.iq_pack_weight_bf3(w.ctypes.data, want.ctypes.data, cout, cin) == 0
    assert lib.iq_split_packed_weight_bf3_host(packed.ctypes.data, got.ctypes.data, cout, cin) == 0, lib.iq_last_error()
    return got, want


@pytest.mark.parametrize("cout,cin", [(4096, 256), (256, 32), (512, 1024), (256, 40)])
def test_split_of_the_packed_image_is_the_packed_split(lib, cout, cin):
    rng = np.random.default_rng(cout + cin)
    got, want = images(lib, rng.standard_normal((cout, cin)).astype(np.float32))
    assert np.array_equal(got, want)
    kp = (cin + 31) // 32 * 32
    terms = got.reshape(3, cout // 32, kp // 16, 64, 8)
    lane, j = np.arange(64)[:, None], np.arange(8)[None, :]
    k = 16 * np.arange(kp // 16)[:, None, None] + 8 * (lane >> 5) + j                  # (k-step, lane, j)
    assert not terms[:, :, k >= cin].any()                                              # zeros where the host image has zeros
    assert terms[0][:, k < cin].any()


def test_split_keeps_every_bit_of_hard_values(lib):
    """Low mantissa bits all set, 60 binades, signed zeros and subnormals (tests/test_hip_parity.py:
    test_bf16x3_split_loses_no_bit_of_a_float32 puts the same kinds of value through the kernel)."""
    rng = np.random.default_rng(9)
    cout, cin = 64, 64
    w = rng.standard_normal((cout, cin)).astype(np.float32)
    w[8:24] = np.ldexp(w[8:24], rng.integers(-30, 31, size=(16, cin))).astype(np.float32)          # 2^-30 .. 2^30
    w[24:40] = (w[24:40].view(np.uint32) | np.uint32(0xffff)).view(np.float32)                      # low 16 mantissa bits set
    w[40:44] = 0.0
    w[44:48] = -0.0
    w[48:56] = (rng.integers(1, 1 << 23, size=(8, cin)).astype(np.uint32) | (rng.integers(0, 2, size=(8, cin)).astype(np.uint32) << 31)).view(np.float32)
    assert np.signbit(w[44:48]).all() and (np.abs(w[48:56]) < np.finfo(np.float32).tiny).all() and (w[48:56] != 0).all()
    got, want = images(lib, w)
    assert np.array_equal(got, want)
    t = (got.astype(np.uint32) << 16).view(np.float32).astype(np.float64).reshape(3, 2, cin // 16, 64, 8).sum(axis=0)
    back = np.empty((cout, cin))
    lane = np.arange(64)
    for nt in range(2):
        for ks in range(cin // 16):
            for j in range(8):
                back[nt * 32 + (lane & 31), 16 * ks + 8 * (lane >> 5) + j] = t[nt, ks, :, j]
    ok = np.ones(cout, dtype=bool)
    ok[48:56] = False                       # (a subnormal's bits below 2^-133, the smallest bf16, belong to no term)
    assert np.array_equal(back[ok], w.astype(np.float64)[ok])                                      # h + m + l = w exactly


def test_split_refuses_a_bad_shape(lib):
    buf = np.zeros(64 * 64, dtype=np.float32)
    out = np.zeros(3 * 64 * 64, dtype=np.uint16)
    assert lib.iq_split_packed_weight_bf3_host(buf.ctypes.data, out.ctypes.data, 64, 12) != 0
    assert b"cin" in lib.iq_last_error()
    assert lib.iq_split_packed_weight_bf3_host(None, out.ctypes.data, 64, 64) != 0
