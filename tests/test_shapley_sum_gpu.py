"""GPU: the sum of iq_shapley_accum / iq_shapley_accum_wide (one workgroup stages sv_rows through LDS, one lane per region adds in
permutation order) against a float64 np.cumsum over the scattered rows - the reference's host loop adds in that order, so the
total and every snapshot must have its bits."""
import numpy as np
import pytest
import torch

from interpret_quality_amd import hip_ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _case(s, r, seed):
    rng = np.random.default_rng(seed)
    orders = np.stack([rng.permutation(r) for _ in range(s)]).astype(np.int64)
    # rewards of mixed sign and magnitude, so that the order of the float64 adds shows in the last bits
    v = (rng.standard_normal((s, r + 1)) * 10.0 ** rng.integers(-3, 4, size=(s, r + 1))).astype(np.float32)
    dv = (v[:, 1:] - v[:, :-1]).astype(np.float32)
    rows = np.zeros((s, r), dtype=np.float64)
    np.put_along_axis(rows, orders, dv.astype(np.float64), axis=1)
    return v, orders, rows


def _check(accum, s, r, counts):
    v, orders, rows = _case(s, r, 1000 * r + s)
    phi, got_rows, snaps = accum(torch.from_numpy(v.reshape(-1)).to(DEV), hip_ops.as_i32(orders, DEV), snap_counts=counts)
    running = np.cumsum(rows, axis=0)                    # sequential float64 adds, row after row
    assert np.array_equal(got_rows.cpu().numpy().view(np.uint64), rows.view(np.uint64))
    assert np.array_equal(phi.cpu().numpy().view(np.uint64), running[-1].view(np.uint64))
    got = snaps.cpu().numpy()
    assert got.shape == (len(counts), r)
    for k, c in enumerate(counts):
        assert np.array_equal(got[k].view(np.uint64), running[c - 1].view(np.uint64)), (s, r, c)


def _counts(s):
    """1, 8 and S, the boundaries of a 64-row piece, and a repeated count."""
    return sorted({c for c in (1, 2, 8, 63, 64, 65, 128, 500, s - 1, s) if 1 <= c <= s}) + [s]


@pytest.mark.parametrize("accum", [hip_ops.shapley_accum, hip_ops.shapley_accum_wide], ids=["narrow", "wide"])
@pytest.mark.parametrize("r", [1, 32, 64])
@pytest.mark.parametrize("s", [1, 7, 8, 9, 1000, 1003])
def test_sum_and_snapshots_equal_a_float64_cumsum_bitwise(s, r, accum):
    _check(accum, s, r, _counts(s))


@pytest.mark.parametrize("s,r", [(9, 65), (130, 130), (67, 1024)])
def test_the_wide_sum_over_several_workgroups(s, r):
    _check(hip_ops.shapley_accum_wide, s, r, _counts(s))


def test_a_single_snapshot_and_none():
    _check(hip_ops.shapley_accum, 1000, 32, [1])
    _check(hip_ops.shapley_accum, 1000, 32, [1000])
    v, orders, rows = _case(70, 32, 3)
    phi, _, snaps = hip_ops.shapley_accum(torch.from_numpy(v.reshape(-1)).to(DEV), hip_ops.as_i32(orders, DEV))
    assert snaps is None and np.array_equal(phi.cpu().numpy().view(np.uint64), np.cumsum(rows, axis=0)[-1].view(np.uint64))
