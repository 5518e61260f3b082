"""GPU: the second moment of the permutation estimator (iq_shapley_sq_accum_games; include/iq.h) against a NumPy loop, bit for bit,
snapshots included - the square of a widened float32 is exact in float64 and the adds run strictly in permutation order, so the
loop has the kernel's bits - and classwise.shapley(se=True) against the column standard error of stage 1's per-permutation rows."""
import argparse
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

import probes
from interpret_quality_amd import _lib, classwise, hip_ops, shapley_stage, synth

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def sq_accum(v, orders, snap_counts):
    """v (G,ldv) float32, orders (S,R) -> (sq (G,R), snaps (G,len(snap_counts),R)) float64: per permutation, in order, the float32
    differences widened, squared and added to the regions they belong to; an entry outside [0, R) is skipped."""
    s, r = orders.shape
    sq = np.zeros((v.shape[0], r))
    snaps = np.zeros((v.shape[0], len(snap_counts), r))
    for o in range(s):
        rows = v[:, o * (r + 1):(o + 1) * (r + 1)]
        dv = (rows[:, 1:] - rows[:, :-1]).astype(np.float64)              # float32 differences, widened
        inside = (orders[o] >= 0) & (orders[o] < r)
        sq[:, orders[o][inside]] += (dv * dv)[:, inside]                     # a permutation names a region once
        for k, count in enumerate(snap_counts):
            if count == o + 1:
                snaps[:, k] = sq
    return sq, snaps


@pytest.mark.parametrize("r", [1, 2, 63, 64, 65, 1024])
@pytest.mark.parametrize("s", [2, 3, 257])
def test_sq_accum_games_is_the_numpy_loop_bit_for_bit(r, s):
    rng = np.random.RandomState(100 * r + s)
    ldv = s * (r + 1) + 3
    v = (2.0 * rng.randn(3, ldv)).astype(np.float32)
    orders = np.stack([rng.permutation(r) for _ in range(s)])
    counts = sorted({1, 2, min(65, s), s})
    want, want_snaps = sq_accum(v, orders, counts)
    vt = torch.from_numpy(v).to(DEV)
    for g in (1, 3):
        sq, snaps = hip_ops.shapley_sq_accum_games(vt[:g], orders, counts)
        assert sq.shape == (g, r) and snaps.shape == (g, len(counts), r) and sq.dtype == torch.float64
        assert np.array_equal(sq.cpu().numpy(), want[:g]) and np.array_equal(snaps.cpu().numpy(), want_snaps[:g]), (r, s, g)
        again, none = hip_ops.shapley_sq_accum_games(vt[:g], hip_ops.as_i32(orders, DEV))
        assert none is None and torch.equal(again, sq)
    total, _ = hip_ops.shapley_accum_games(vt, orders)                       # the sibling keeps its bits beside the new entry
    rows = np.stack([(v[:, o * (r + 1) + 1:(o + 1) * (r + 1)] - v[:, o * (r + 1):(o + 1) * (r + 1) - 1]).astype(np.float64)[:, np.argsort(orders[o])]
                     for o in range(s)])
    run = np.zeros((3, r))
    for o in range(s):
        run += rows[o]
    assert np.array_equal(total.cpu().numpy(), run)
    se = hip_ops.shapley_se(total, sq, s)
    assert se.shape == (3, r) and np.all(np.isfinite(se)) and np.all(se >= 0)


def test_an_order_entry_outside_the_regions_is_skipped():
    r, s = 70, 3
    rng = np.random.RandomState(9)
    v = rng.randn(2, s * (r + 1)).astype(np.float32)
    orders = np.stack([rng.permutation(r) for _ in range(s)])
    orders[1, 5], orders[2, 0] = r, -1
    want, _ = sq_accum(v, orders, [])
    got, _ = hip_ops.shapley_sq_accum_games(torch.from_numpy(v).to(DEV), hip_ops.as_i32(orders, DEV), validate=False)
    assert np.array_equal(got.cpu().numpy(), want)
    with pytest.raises(_lib.IqError):
        hip_ops.shapley_sq_accum_games(torch.from_numpy(v).to(DEV), orders)      # the host check of the ndarray form
    with pytest.raises(_lib.IqError):
        hip_ops.shapley_se(np.zeros(3), np.zeros(3), 1)


def _ulps(got, want):
    return np.abs(got - want) / np.spacing(np.abs(want))


def test_classwise_se_is_the_column_standard_error_of_stage_1_rows():
    pts, y = synth.make_cloud(0, 128)
    data = torch.from_numpy(np.ascontiguousarray(pts))[None].to(DEV)
    fps = hip_ops.fps(data, 8)[0].contiguous()
    rid = hip_ops.region_assign_wide(data[0].contiguous(), fps).cpu().numpy().astype(np.int64)
    args = argparse.Namespace(model="pointnet", softmax_type="modified", num_points=128, num_regions=8, verbose=False)
    model, _ = probes.coalition_model("pointnet", DEV)
    orders = np.stack([np.random.RandomState(11).permutation(8) for _ in range(4)])
    snaps, total, se = classwise.shapley(model, data, rid, orders, args, snap_counts=[1, 4], se=True)
    plain_snaps, plain = classwise.shapley(model, data, rid, orders, args, snap_counts=[1, 4])
    assert np.array_equal(total, plain) and all(np.array_equal(snaps[k], plain_snaps[k]) for k in (1, 4))
    assert se.shape == total.shape and se.dtype == np.float64
    _, rows, want_total = shapley_stage.shapley_all_orders(model, data, torch.tensor([int(y)], device=DEV), rid, orders, args)
    rows = np.asarray(rows.cpu() if isinstance(rows, torch.Tensor) else rows, dtype=np.float64)
    assert rows.shape == (4, 8) and np.array_equal(total[int(y)], want_total)
    want = np.zeros(8)                                                        # the column standard error in rationals, rounded at the end
    for k in range(8):
        col = [Fraction(float(x)) for x in rows[:, k]]
        mean = sum(col) / 4
        want[k] = math.sqrt(sum((x - mean) ** 2 for x in col) / 3 / 4)
    ulps = _ulps(se[int(y)], want)
    print("se of the ground-truth class against the column standard error: %s ulp" % np.array2string(ulps, precision=2))
    assert np.all(ulps <= 4.0)
    assert np.all(np.isfinite(se)) and np.all(se >= 0)
    with pytest.raises(_lib.IqError):
        classwise.shapley(model, data, rid, orders[:1], args, se=True)

