"""GPU: wide games - coalitions over more than 64 regions, up to one region per point (include/iq.h "Wide coalitions",
interpret_quality_amd/wide.py, final_wide_shapley.py).

Bars (none is new):
  * masks, region ids, fused = dense on materialised clouds, wide = narrow at R <= 64, batch independence, running sums: bitwise;
  * logits against the CPU oracle: 1e-4 (conftest.assert_close_elementwise for PointNet, probes.COALITION_RTOL of max |logit|
    for the other families; DGCNN keeps its qualified bar: the bitwise identity only);
  * Shapley values against oracle.shap_sampling_stage1 - at R = 128 and with one region per point (N = R = 256, 1024): the total
    and the per-permutation rows 1e-4 norm-wise;
  * efficiency of a permutation row: R float32 roundings of at most 2 max|v| 2^-24 each (the row is summed with math.fsum, so the
    check adds no rounding of its own).
"""
import argparse
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import probes
from conftest import REPO, assert_close_elementwise
from interpret_quality_amd import _lib, final_common, hip_ops, synth, wide
from oracle import ref_cpu

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _args(family="pointnet", num_regions=128, num_points=1024):
    return argparse.Namespace(model=family, softmax_type="modified", num_points=num_points, num_regions=num_regions, verbose=False)


def _random_keep(rng, b, r):
    """(b, W) uint64 rows: coalition sizes spread over 0 .. R, the first row full, the last empty; bits at and above R are noise."""
    w = (r + 63) // 64
    member = rng.random((b, w * 64)) < rng.random((b, 1))
    member[0, :], member[-1, :] = True, False
    member[:, r:] = rng.random((b, w * 64 - r)) < 0.5
    weights = np.left_shift(np.uint64(1), (np.arange(w * 64) & 63).astype(np.uint64))
    return np.where(member, weights, np.uint64(0)).reshape(b, w, 64).sum(axis=2, dtype=np.uint64), member[:, :r]


def _cloud(i, n=1024):
    pts, y = synth.make_cloud(i, n)
    return torch.from_numpy(pts)[None], torch.tensor([y])


def _fps_regions(data, r):
    """Region ids of the oracle for the oracle's FPS centres: (N,) int64."""
    fps = ref_cpu.farthest_point_sample(data, r)[0].numpy()
    return np.asarray(ref_cpu.cal_region_id(data, fps)).astype(np.int64)


# ---- 1. masks ----

@pytest.mark.parametrize("n", [1000, 1024, 2500])
@pytest.mark.parametrize("r", [65, 128, 200, 1024])
def test_prefix_masks_and_masking_are_bit_exact(r, n):
    rng = np.random.default_rng(100 * r + n)
    data, _ = _cloud(7, n)
    center = data.mean(dim=1).squeeze()
    rid = rng.integers(0, r, size=n)
    rid[rid == 7] = 8                                           # region 7 is empty
    orders = np.stack([rng.permutation(r) for _ in range(3)])
    bad = orders[2].copy()
    bad[r // 3] = r + 5                                        # an out-of-range entry: ignored, its region is never kept
    want = ref_cpu.shapley_masked_batch(data, center, orders[:2], rid)
    keep_bad = np.stack([np.isin(rid, bad[:i][bad[:i] < r]) for i in range(r + 1)])
    want_bad = torch.where(torch.from_numpy(keep_bad)[:, :, None], data.expand(r + 1, n, 3), center.reshape(1, 1, 3).expand(r + 1, n, 3))
    want = torch.cat([want, want_bad], dim=0)
    dev_orders = hip_ops.as_i32(np.stack([orders[0], orders[1], bad]), DEV)
    keep = hip_ops.prefix_keep_masks_wide(dev_orders)
    assert keep.shape == (3 * (r + 1), (r + 63) // 64)
    host = wide.prefix_keep_masks(np.stack([orders[0], orders[1], bad]), r)
    assert np.array_equal(keep.cpu().numpy().view(np.uint64), host)
    cloud, ridt, c = data[0].to(DEV).contiguous(), hip_ops.as_i32(rid, DEV), center.to(DEV).contiguous()
    got = hip_ops.mask_coalitions_wide(cloud, ridt, keep, c, r, channel_first=False)
    assert got.shape == (3 * (r + 1), n, 3) and torch.equal(got.cpu(), want)
    got_cf = hip_ops.mask_coalitions_wide(cloud, ridt, keep, c, r, channel_first=True)
    assert got_cf.shape == (3 * (r + 1), 3, n) and torch.equal(got_cf.cpu(), want.permute(0, 2, 1))


def test_wide_wrappers_refuse_bad_arguments():
    data, _ = _cloud(0)
    cloud = data[0].to(DEV).contiguous()
    rid = torch.zeros((1024,), dtype=torch.int32, device=DEV)
    c = torch.zeros((3,), device=DEV)
    with pytest.raises(_lib.IqError):
        hip_ops.mask_coalitions_wide(cloud, rid, torch.zeros((4, 1), dtype=torch.int64, device=DEV), c, 128)     # W must be 2
    with pytest.raises(_lib.IqError):
        hip_ops.prefix_keep_masks_wide(torch.zeros((1, 1025), dtype=torch.int32, device=DEV))
    with pytest.raises(_lib.IqError):
        hip_ops.region_assign_wide(cloud, torch.zeros((1025,), dtype=torch.int32, device=DEV))


# ---- 2. region ids ----

@pytest.mark.parametrize("r", [65, 256, 1024])
def test_region_ids_are_bit_exact(r):
    for i in (0, 5):
        data, _ = _cloud(i)
        fps = hip_ops.fps(data.to(DEV), r)[0].contiguous()
        got = hip_ops.region_assign_wide(data[0].to(DEV).contiguous(), fps).cpu().numpy()
        want = ref_cpu.cal_region_id(data, fps.cpu().numpy())
        assert np.array_equal(got, want)
        if r == 1024:
            assert np.array_equal(np.sort(got), np.arange(1024))     # distinct points: every point is its own region


@pytest.mark.parametrize("r", [1, 32, 64])
def test_region_ids_equal_the_narrow_kernel_up_to_64_regions(r):
    data, _ = _cloud(2)
    fps = hip_ops.fps(data.to(DEV), r)[0].contiguous()
    cloud = data[0].to(DEV).contiguous()
    assert torch.equal(hip_ops.region_assign_wide(cloud, fps), hip_ops.region_assign(cloud, fps))


# ---- 3. PointNet ----

def _pointnet_inputs(r, nc=1, n=1024, per_point=False):
    clouds = torch.cat([_cloud(i, n)[0] for i in range(nc)], dim=0)
    if per_point:
        rid = np.stack([np.random.default_rng(i).permutation(n) for i in range(nc)])
    else:
        rid = np.stack([_fps_regions(clouds[i:i + 1], r) for i in range(nc)])
    return clouds.to(DEV).contiguous(), clouds.mean(dim=1).to(DEV).contiguous(), hip_ops.as_i32(rid, DEV)


@pytest.mark.parametrize("r", [32, 64])
def test_pointnet_wide_equals_narrow_bitwise_up_to_64_regions(r):
    model, _ = probes.coalition_model("pointnet", DEV)
    clouds, centers, rid = _pointnet_inputs(r, nc=2)
    rng = np.random.default_rng(r)
    keep, _ = _random_keep(rng, 500, r)
    cloud_of = torch.from_numpy(rng.integers(0, 2, size=500).astype(np.int32)).to(DEV)
    kw = hip_ops.wide_masks_to_tensor(keep, DEV)
    narrow = model.coalition_logits(clouds, centers, rid, kw[:, 0].contiguous(), cloud_of, num_regions=r)
    got = model.coalition_logits_wide(clouds, centers, rid, kw, cloud_of, num_regions=r)
    assert torch.equal(got, narrow)


@pytest.mark.parametrize("r,per_point", [(128, False), (1024, True)])
def test_pointnet_wide_fused_equals_dense_on_materialised_clouds_bitwise(r, per_point):
    model, _ = probes.coalition_model("pointnet", DEV)
    clouds, centers, rid = _pointnet_inputs(r, per_point=per_point)
    keep, _ = _random_keep(np.random.default_rng(r), 300, r)
    kw = hip_ops.wide_masks_to_tensor(keep, DEV)
    got = model.coalition_logits_wide(clouds, centers, rid, kw, None, num_regions=r)
    masked = hip_ops.mask_coalitions_wide(clouds[0].contiguous(), rid[0].contiguous(), kw, centers[0].contiguous(), r, channel_first=True)
    dense = model(masked)[0]
    assert got.shape == (300, 10) and torch.isfinite(got).all()
    assert torch.equal(got, dense)


def test_pointnet_wide_matches_the_oracle_on_200_coalitions():
    r = 128
    model, sd = probes.coalition_model("pointnet", DEV)
    clouds, centers, rid = _pointnet_inputs(r)
    keep, member = _random_keep(np.random.default_rng(3), 200, r)
    got = model.coalition_logits_wide(clouds, centers, rid, hip_ops.wide_masks_to_tensor(keep, DEV), None, num_regions=r).cpu().numpy()
    pts, c = clouds[0].cpu(), centers[0].cpu()
    kept = torch.from_numpy(member[:, rid[0].cpu().numpy()])[:, :, None]
    masked = torch.where(kept, pts[None].expand(200, 1024, 3), c.reshape(1, 1, 3).expand(200, 1024, 3)).contiguous()
    want = probes.oracle_logits("pointnet", sd, masked)
    print("pointnet R=128 vs oracle: max |d| / max |logit| = %.3g" % probes.rel_max_err(got, want))
    assert_close_elementwise(got, want, rtol=1e-4)


def test_pointnet_wide_logits_do_not_depend_on_the_launch():
    r = 128
    model, _ = probes.coalition_model("pointnet", DEV)
    clouds, centers, rid = _pointnet_inputs(r)
    keep, _ = _random_keep(np.random.default_rng(4), 4000, r)
    kw = hip_ops.wide_masks_to_tensor(keep, DEV)
    big = model.coalition_logits_wide(clouds, centers, rid, kw, None, num_regions=r)
    for i in (0, 1234, 3999):
        assert torch.equal(model.coalition_logits_wide(clouds, centers, rid, kw[i:i + 1].contiguous(), None, num_regions=r), big[i:i + 1])
    # the same batch over several launches (the split the free memory would ask for)
    cap = type(model).max_wide_per_call
    try:
        type(model).max_wide_per_call = 1500
        assert torch.equal(model.coalition_logits_wide(clouds, centers, rid, kw, None, num_regions=r), big)
    finally:
        type(model).max_wide_per_call = cap


# ---- 4. the other families ----

@pytest.mark.parametrize("family", ["pointnet2", "gcnn", "pointconv", "dgcnn"])
def test_other_families_run_wide_coalitions_through_their_dense_forward(family):
    r = 128
    model, sd = probes.coalition_model(family, DEV)
    data, _ = _cloud(1)
    rid = _fps_regions(data, r)
    keep, _ = _random_keep(np.random.default_rng(5), 40, r)
    d = data.to(DEV)
    got = wide.coalition_logits(model, d, rid, keep, _args(family, r))
    masked = hip_ops.mask_coalitions_wide(d[0].contiguous(), hip_ops.as_i32(rid, DEV), hip_ops.wide_masks_to_tensor(keep, DEV),
                                          d.mean(dim=1).reshape(3).contiguous(), r)
    assert got.shape == (40, 10) and torch.equal(got, model.forward_points(masked))
    if family != "dgcnn":       # DGCNN's bar against the float32 oracle is qualified (dynamic graphs): the bitwise identity only
        want = probes.oracle_logits(family, sd, masked.cpu())
        err = probes.rel_max_err(got.cpu().numpy(), want)
        print("%s R=128 vs oracle: max |d| / max |logit| = %.3g" % (family, err))
        assert err <= probes.COALITION_RTOL


# ---- 5. Shapley values ----

_SHAP = {}


def _shapley_128():
    """PointNet, R = 128, 20 permutations: the API result and what it was computed from."""
    if not _SHAP:
        r = 128
        data, lbl = _cloud(0)
        rid = _fps_regions(data, r)
        orders = synth.make_orders(20, r, seed=2)
        model, sd = probes.coalition_model("pointnet", DEV)
        snaps, rows, total = wide.shapley(model, data.to(DEV), lbl.to(DEV), rid, orders, _args("pointnet", r), snap_counts=[10, 20])
        _SHAP.update(data=data, lbl=lbl, rid=rid, orders=orders, sd=sd, snaps=snaps, rows=rows, total=total)
    return _SHAP


def _norm_rel(got, want):
    return float(np.linalg.norm(np.asarray(got) - np.asarray(want)) / np.linalg.norm(np.asarray(want)))


def test_shapley_values_at_128_regions_match_the_oracle():
    s = _shapley_128()
    want_total, want_rows = ref_cpu.shap_sampling_stage1(ref_cpu.PointNetOracle(s["sd"]), s["data"], s["lbl"], s["rid"], s["orders"], 128)
    e_total, e_rows = _norm_rel(s["total"], want_total), _norm_rel(s["rows"], want_rows)
    print("R=128, 20 permutations: total rel %.3g, rows rel %.3g" % (e_total, e_rows))
    assert s["rows"].shape == (20, 128) and s["rows"].dtype == np.float64 and s["total"].shape == (128,)
    assert e_total <= 1e-4
    assert e_rows <= 1e-4


def test_running_sums_are_the_partial_sums_of_the_rows_bitwise():
    s = _shapley_128()
    acc = np.zeros((128,))
    for o in range(20):
        acc += s["rows"][o]
        if o + 1 in (10, 20):
            assert np.array_equal(s["snaps"][o + 1], acc)
    assert np.array_equal(s["total"], acc) and sorted(s["snaps"]) == [10, 20]


def _efficiency(rows, v, r):
    """Every permutation's row sums to v(full) - v(empty): R float32 roundings of at most 2 max|v| 2^-24 each."""
    v = v.reshape(-1, r + 1).astype(np.float64)
    vmax = float(np.abs(v).max())
    bound = r * 2 * vmax * 2.0 ** -24
    gap = np.array([abs(math.fsum(list(row) + [-vs[-1], vs[0]])) for row, vs in zip(rows, v)])
    print("efficiency: worst gap / bound = %.3g" % float(gap.max() / bound))
    assert np.all(gap <= bound), (gap, bound)


def test_every_permutation_row_sums_to_v_full_minus_v_empty():
    s = _shapley_128()
    model, _ = probes.coalition_model("pointnet", DEV)
    args = _args("pointnet", 128)
    keep = hip_ops.prefix_keep_masks_wide(hip_ops.as_i32(s["orders"], DEV))
    logits = wide.coalition_logits(model, s["data"].to(DEV), s["rid"], keep, args)
    v = final_common.get_reward(logits, s["lbl"].to(DEV), args).cpu().numpy()
    assert np.all(v.reshape(20, 129)[:, 0] == v[0]) and np.all(v.reshape(20, 129)[:, -1] == v[128])
    _efficiency(s["rows"], v, 128)


def test_shapley_accum_wide_equals_the_narrow_kernel_at_64_regions():
    r, s = 64, 37
    rng = np.random.default_rng(9)
    v = torch.from_numpy(rng.standard_normal(s * (r + 1)).astype(np.float32) * 5).to(DEV)
    orders = hip_ops.as_i32(np.stack([rng.permutation(r) for _ in range(s)]), DEV)
    a = hip_ops.shapley_accum(v, orders, snap_counts=[1, 10, 36, 37])
    b = hip_ops.shapley_accum_wide(v, orders, snap_counts=[1, 10, 36, 37])
    for x, y in zip(a, b):
        assert torch.equal(x, y)


# ---- 6. one region per point ----

@pytest.mark.parametrize("n,perms", [(256, 4), (1024, 1)])
def test_point_level_shapley_values_match_the_oracle(n, perms):
    data, lbl = _cloud(0, n)
    fps = hip_ops.fps(data.to(DEV), n)[0].contiguous()
    rid = hip_ops.region_assign_wide(data[0].to(DEV).contiguous(), fps).cpu().numpy().astype(np.int64)
    assert np.array_equal(np.sort(rid), np.arange(n))
    orders = synth.make_orders(perms, n, seed=3)
    model, sd = probes.coalition_model("pointnet", DEV)
    args = _args("pointnet", n, n)
    _, rows, total = wide.shapley(model, data.to(DEV), lbl.to(DEV), rid, orders, args)
    want_total, want_rows = ref_cpu.shap_sampling_stage1(ref_cpu.PointNetOracle(sd), data, lbl, rid, orders, n)
    e_total, e_rows = _norm_rel(total, want_total), _norm_rel(rows, want_rows)
    print("N=R=%d, %d permutation(s): total rel %.3g, rows rel %.3g, max |d marginal| %.3g, max |marginal| %.3g" % (
        n, perms, e_total, e_rows, float(np.abs(rows - want_rows).max()), float(np.abs(want_rows).max())))
    assert rows.shape == (perms, n) and total.shape == (n,)
    assert e_total <= 1e-4
    assert e_rows <= 1e-4


def test_players_of_empty_regions_get_exactly_zero():
    pts, y = synth.make_cloud(4)
    pts = pts.copy()
    pts[1008:] = pts[:16]                                        # 16 duplicated points
    data, lbl = torch.from_numpy(pts)[None], torch.tensor([y])
    fps = hip_ops.fps(data.to(DEV), 1024)[0].contiguous()
    rid = hip_ops.region_assign_wide(data[0].to(DEV).contiguous(), fps).cpu().numpy().astype(np.int64)
    assert np.array_equal(rid, ref_cpu.cal_region_id(data, fps.cpu().numpy()))
    empty = np.setdiff1d(np.arange(1024), rid)
    assert len(empty) == 16                                     # FPS repeats index 0 once the distinct locations are used up
    orders = synth.make_orders(3, 1024, seed=4)
    model, _ = probes.coalition_model("pointnet", DEV)
    _, rows, total = wide.shapley(model, data.to(DEV), lbl.to(DEV), rid, orders, _args("pointnet", 1024))
    assert np.all(rows[:, empty] == 0.0) and np.all(total[empty] == 0.0)
    assert np.isfinite(rows).all() and np.count_nonzero(rows) > 1024


# ---- 7. the driver ----

def _env():
    env = dict(os.environ, PYTHONPATH=REPO)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "IQ_FORCE_DIST", "IQ_REHEARSAL"):
        env.pop(k, None)
    return env


def _run_script(script, extra, cwd):
    import gc
    gc.collect()
    torch.cuda.empty_cache()            # the child shares this GPU: hand back what the caching allocator holds
    cmd = [sys.executable, os.path.join(REPO, script), "--model", "pointnet", "--dataset", "modelnet10", "--synthetic", "--num_clouds", "1",
           "--num_samples_save", "10"] + extra
    return subprocess.run(cmd, cwd=str(cwd), env=_env(), capture_output=True, text=True, timeout=600)


def test_final_wide_shapley_script_end_to_end(tmp_path):
    r = _run_script("final_wide_shapley.py", ["--num_regions", "128"], tmp_path)
    assert r.returncode == 0, r.stderr[-3000:]
    root = tmp_path / "checkpoints" / "exp_MODEL_pointnet_DATA_modelnet10_POINTNUM_1024_REGIONNUM_128_shapley_test" / "synthetic_00"
    region_id, all_orders = np.load(root / "region_id.npy"), np.load(root / "all_orders.npy")
    sv = np.load(root / "region_sv_all.npy")
    assert region_id.shape == (1024,) and region_id.dtype == np.int64 and region_id.min() == 0 and region_id.max() == 127
    assert np.load(root / "norm_factor.npy").shape == ()
    assert all_orders.shape == (10, 128) and np.array_equal(all_orders, synth.make_orders(10, 128, seed=1))
    assert sv.shape == (10, 128) and sv.dtype == np.float64
    assert (tmp_path / "fps_modelnet10_1024_128_index_final30.npy").exists()
    # the API on the same cloud, regions and permutations: the same bits
    data, lbl = _cloud(0)
    model, _ = probes.coalition_model("pointnet", DEV)
    _, rows, _ = wide.shapley(model, data.to(DEV), lbl.to(DEV), region_id, all_orders, _args("pointnet", 128))
    assert np.array_equal(rows, sv)


def test_final_wide_shapley_writes_stage_one_snapshots(tmp_path, monkeypatch):
    """100 permutations reach the first of stage 1's sample counts: shapley/<i>_100.npy and region_shapley/<i>_100.npy."""
    from interpret_quality_amd import wide_stage
    monkeypatch.chdir(tmp_path)
    wide_stage.main(["--model", "pointnet", "--dataset", "modelnet10", "--synthetic", "--num_clouds", "1", "--num_samples_save", "100",
                     "--num_regions", "65"])
    root = tmp_path / "checkpoints" / "exp_MODEL_pointnet_DATA_modelnet10_POINTNUM_1024_REGIONNUM_65_shapley_test" / "synthetic_00"
    sv, rid = np.load(root / "region_sv_all.npy"), np.load(root / "region_id.npy")
    region, point = np.load(root / "region_shapley" / "0_100.npy"), np.load(root / "shapley" / "0_100.npy")
    assert sv.shape == (100, 65) and region.shape == (65,) and point.shape == (1024,)
    acc = np.zeros((65,))
    for row in sv:
        acc += row
    assert np.array_equal(region, acc / 100) and np.array_equal(point, region[rid])


def test_final_shapley_value_still_refuses_65_regions(tmp_path):
    """The narrow stage was left alone: more than 64 regions are still an error there."""
    r = _run_script("final_shapley_value.py", ["--num_regions", "65"], tmp_path)
    assert r.returncode != 0
    assert not list(tmp_path.glob("checkpoints/*/synthetic_00/region_sv_all.npy"))
