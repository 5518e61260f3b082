"""GPU: the bf16x3 dense layer (pn_gemm_bf3_kernel<false>, pn_gemm_bf3_short_kernel) with the tile heights launch_linear chooses for
iq_linear and PointNet's heads - 128-row
workgroups in whole rounds of 2 x CUs, 32- / 64-row ones throughout for a launch below one / two rounds and for the rows of a
nearly empty last round - against the same layer on 128-row tiles only (twin "dense_tile128", the former launch): bit for bit, for every row count
around the tile edges and around the rounds of THIS device.  Each case also holds what
test_hip_parity.py::test_dense_layer_on_the_bf16_matrix_pipe_is_float32_exact holds (its bars against a float64 product, a
row's result independent of the launch it is in), and that the C entry writes no row beyond M.

The device split of a float32 weight image into the bf16x3 image (iq_split_packed_weight_bf3) against the host packer."""
import ctypes

import numpy as np
import pytest
import torch

from interpret_quality_amd import _lib, hip_ops
from interpret_quality_amd.tuning import tuned

pytestmark = pytest.mark.gpu

LAYERS = [(1024, 512, 1), (512, 256, 1), (256, 4096, 0), (40, 256, 0)]          # (cin, cout, act); the last: the ragged instantiation
FIXED_M = [1, 31, 32, 33, 63, 64, 65, 96, 127, 128, 129, 191, 193, 257, 700]
SENTINEL = 0x7fc12345                                                            # a NaN no kernel computes


def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def rel_err(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


_LAYERS = {}


def layer_of(cin, cout):
    """(PackedLinear with the bf16x3 image, w, b) of a seeded layer: packed once per process."""
    if (cin, cout) not in _LAYERS:
        rng = np.random.default_rng(1000 * cin + cout)
        w = (rng.standard_normal((cout, cin)) / np.sqrt(cin)).astype(np.float32)
        b = rng.standard_normal(cout).astype(np.float32)
        _LAYERS[(cin, cout)] = (hip_ops.PackedLinear(w, b, dev(), bf3=True), w, b)
    return _LAYERS[(cin, cout)]


def check_case(m, cin, cout, act):
    layer, w, b = layer_of(cin, cout)
    d = dev()
    x = np.random.default_rng(m + cin).standard_normal((m, cin)).astype(np.float32)
    xt = torch.from_numpy(x).to(d)
    got = hip_ops.linear(xt, layer, act)
    former = tuned("dense_tile128", lambda: hip_ops.linear(xt, layer, act))
    assert torch.equal(got, former), "M=%d: %d values differ from the 128-row launch" % (m, int((got != former).sum()))
    k = min(m, 77)
    assert torch.equal(hip_ops.linear(xt[:k].contiguous(), layer, act), got[:k])          # launch-size independent
    f32 = tuned("dense_fp32", lambda: hip_ops.linear(xt, layer, act))
    ref = torch.from_numpy(x).double() @ torch.from_numpy(w).double().T + torch.from_numpy(b).double()
    if act == 1:
        ref = torch.relu(ref)
    e_bf3, e_f32 = rel_err(got.cpu().numpy(), ref.numpy()), rel_err(f32.cpu().numpy(), ref.numpy())
    print("M=%d %d -> %d: e_bf3 %.3g e_f32 %.3g" % (m, cin, cout, e_bf3, e_f32))
    assert e_bf3 < 2e-6 and e_bf3 <= 1.5 * e_f32 + 1e-7, (e_bf3, e_f32)
    # the C entry on a buffer 256 rows longer than M: nothing beyond row M is written
    buf = torch.full(((m + 256) * cout,), SENTINEL, dtype=torch.int32, device=d)
    lib = _lib.load()
    _lib.check(lib.iq_linear(xt.data_ptr(), cin, ctypes.byref(layer.struct), buf.data_ptr(), cout, m, act, hip_ops._stream()), "iq_linear")
    torch.cuda.synchronize()
    assert torch.equal(buf[:m * cout].view(torch.float32).view(m, cout), got)
    assert bool((buf[m * cout:] == SENTINEL).all()), "M=%d: rows beyond M written" % m


@pytest.mark.parametrize("m", FIXED_M)
@pytest.mark.parametrize("cin,cout,act", LAYERS)
def test_short_tiles_equal_the_128_row_launch(cin, cout, act, m):
    check_case(m, cin, cout, act)


def round_cases():
    """Row counts around the rounds of this device (a round = 2 x CUs workgroups of 128 rows; cin = 64, act 1):
    one workgroup over a round at one column block, one row tile over it at two, and the last row count below a round - each with
    one tile less and more (32-row tiles below one round, 64-row tiles below two); one workgroup / one row tile over TWO rounds at
    one / two column blocks, with one tile less and more (128-row tiles, the rows of a last round a quarter full or less on 32-row
    tiles behind them); a third round three eighths full (64-row tiles behind the whole rounds) and one three quarters full
    (128-row tiles throughout)."""
    rnd = 2 * torch.cuda.get_device_properties(0).multi_processor_count
    out = []
    for cout, m in ((256, rnd * 128 + 1), (512, rnd // 2 * 128 + 1), (256, (rnd - 1) * 128 + 1), (256, 2 * rnd * 128 + 1), (512, rnd * 128 + 1)):
        out += [(64, cout, m + dm) for dm in (-128, 0, 128)]
    return out + [(64, 256, (2 * rnd + 3 * rnd // 8) * 128 - 5), (64, 256, (2 * rnd + 3 * rnd // 4) * 128 + 9)]


N_ROUND_CASES = 17


@pytest.mark.parametrize("i", range(N_ROUND_CASES))
def test_row_counts_around_the_rounds_of_this_device(i):
    cases = round_cases()
    assert len(cases) == N_ROUND_CASES
    cin, cout, m = cases[i]
    check_case(m, cin, cout, 1)


def test_33000_rows_of_the_512_to_256_head():
    check_case(33000, 512, 256, 1)


def test_device_split_of_the_packed_image_equals_the_host_packer():
    lib = _lib.load()
    cout, cin = 4096, 256
    w = np.random.default_rng(4096 + 256).standard_normal((cout, cin)).astype(np.float32)
    packed = np.empty(lib.iq_packed_floats(cout, cin), dtype=np.float32)
    assert lib.iq_pack_weight(w.ctypes.data, packed.ctypes.data, cout, cin) == 0
    want = np.empty(lib.iq_packed_bf3_elems(cout, cin), dtype=np.uint16)
    assert lib.iq_pack_weight_bf3(w.ctypes.data, want.ctypes.data, cout, cin) == 0
    pt = torch.from_numpy(packed).to(dev())
    out = torch.full((want.size,), 0x1234, dtype=torch.int16, device=dev())
    _lib.check(lib.iq_split_packed_weight_bf3(pt.data_ptr(), out.data_ptr(), cout, cin, hip_ops._stream()), "iq_split_packed_weight_bf3")
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint16), want)
