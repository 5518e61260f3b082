"""GPU: the smoothness enumeration of wide games (iq_smoothness_enum_wide, hip_ops.smoothness_enum_wide,
smoothness.enumerate_smoothness(wide=True), final_wide_smoothness.py).

The wide entry launches the narrow entry's kernel, one wave per region, and a region's trajectory reads only that region's points.
So: at R <= 64 all five outputs are the narrow entry's, compared as raw bits (NaNs count); above 64 regions every region of a
63-region window equals, bitwise, the narrow run on the relabelled cloud (window -> regions 0 .. 62, every other point -> region 63)
- which ties the wide entry to the kernel the reference's goldens pin (tests/test_smoothness_gpu.py); and against the CPU oracle
the bars are that file's (orig 1e-6, ATOL_SMOOTH, ATOL_DATA) on its unbounded three-epoch trajectories, at R = 65 where no region
is degenerate.
"""
import argparse

import numpy as np
import pytest
import torch

import probes
import wide_drivers as wd
from conftest import load_golden
from interpret_quality_amd import _lib, hip_ops, smoothness, synth, wide
from oracle import ref_cpu
from test_smoothness_gpu import ATOL_DATA, ATOL_SMOOTH, enum_args

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
OUTPUTS = ("data", "smoothness", "var", "orig", "stop_epoch")
_FPS = {}


def _cloud(i, n=1024):
    return torch.from_numpy(synth.make_cloud(i, n)[0])[None]


def _fps_regions(i, r):
    """FPS regions of synthetic cloud i (the oracle's centres and ids), (1024,) int64."""
    if (i, r) not in _FPS:
        data = _cloud(i)
        _FPS[(i, r)] = np.asarray(ref_cpu.cal_region_id(data, ref_cpu.farthest_point_sample(data, r)[0].numpy())).astype(np.int64)
    return _FPS[(i, r)]


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---- 1. wide equals narrow up to 64 regions ----

@pytest.mark.parametrize("mode,objective", [("linearity", "inc"), ("scattering", "dec")])
@pytest.mark.parametrize("source,r", [("golden", 32), ("golden", 64), ("fps", 32), ("fps", 64)])
def test_wide_entry_equals_the_narrow_entry_bitwise_up_to_64_regions(source, r, mode, objective):
    """golden at R = 64: the golden's 32 regions with 32 empty ones declared behind them."""
    cloud = _cloud(2 if source == "golden" else 4)[0].to(DEV).contiguous()
    rid = hip_ops.as_i32(load_golden("smoothness.npz")["region_id"] if source == "golden" else _fps_regions(4, r), DEV)
    narrow = hip_ops.smoothness_enum(cloud, rid, r, mode, objective)
    got = hip_ops.smoothness_enum_wide(cloud, rid, r, mode, objective)
    assert narrow["stop_epoch"].max().item() > 0             # something moved
    for k in OUTPUTS:
        assert got[k].shape == narrow[k].shape and torch.equal(_bits(got[k]), _bits(narrow[k])), k


# ---- 2. per-region independence above 64 regions ----

@pytest.mark.parametrize("r,mode,objective", [(128, "planarity", "inc"), (256, "linearity", "dec")])
def test_every_region_of_a_window_equals_the_narrow_run_on_the_relabelled_cloud(r, mode, objective):
    rid = _fps_regions(2, r).copy()
    sizes = np.bincount(rid, minlength=r)
    if r == 128:
        assert sizes.min() == 2 and sizes.max() == 23
    else:
        assert int((sizes == 1).sum()) == 15
    rid[rid == 70] = 71                                       # region 70 is empty (second window)
    cloud = _cloud(2)[0].to(DEV).contiguous()
    wide_res = {k: v.cpu().numpy() for k, v in hip_ops.smoothness_enum_wide(cloud, hip_ops.as_i32(rid, DEV), r, mode, objective).items()}
    assert wide_res["stop_epoch"][70] == -1 and wide_res["stop_epoch"].max() > 0
    for lo in (0, 33, r - 63):                                # the first window, the one that holds region 64, the last
        inside = (rid >= lo) & (rid < lo + 63)
        local = np.where(inside, rid - lo, 63)
        nar = {k: v.cpu().numpy() for k, v in hip_ops.smoothness_enum(cloud, hip_ops.as_i32(local, DEV), 64, mode, objective).items()}
        win = slice(lo, lo + 63)
        assert np.array_equal(nar["smoothness"][:, :63].view(np.int32), wide_res["smoothness"][:, win].view(np.int32))
        assert np.array_equal(nar["var"][:, :63].view(np.int32), wide_res["var"][:, win].view(np.int32))
        assert np.array_equal(nar["orig"][:63].view(np.int32), wide_res["orig"][win].view(np.int32))
        assert np.array_equal(nar["stop_epoch"][:63], wide_res["stop_epoch"][win])
        assert np.array_equal(nar["data"][:, inside].view(np.int32), wide_res["data"][:, inside].view(np.int32))


# ---- 3. against the CPU oracle ----

@pytest.mark.parametrize("cloud,mode,objective", [(2, "planarity", "inc"), (4, "linearity", "dec")])
def test_unbounded_trajectories_at_65_regions_match_the_oracle(cloud, mode, objective):
    """tests/test_smoothness_gpu.py::test_unbounded_trajectories_match_oracle at R = 65 (region sizes 5 .. 36 and 6 .. 30, no
    region with a relative eigenvalue gap below 1e-2): every region is compared."""
    data = _cloud(cloud)
    rid = _fps_regions(cloud, 65)
    kw = dict(var_threshold=1e9, dist_threshold=1e9, epoch=3)
    want_d, want_s, want_o = ref_cpu.smoothness_enumerate(data, rid, 65, mode, objective, **kw)
    poses, sm, res = smoothness.enumerate_smoothness(data.to(DEV), rid, enum_args(mode, num_regions=65, **kw), objective, wide=True)
    assert poses.shape[0] == want_d.shape[0] == 3 and sm.shape == want_s.shape == (3, 65)
    e_orig = np.abs(res["orig"].cpu().numpy() - want_o).max()
    e_sm, e_data = np.abs(sm - want_s).max(), np.abs(poses.cpu().numpy() - want_d[:, 0]).max()
    print("cloud %d %s %s: orig %.3g, smoothness %.3g, data %.3g" % (cloud, mode, objective, e_orig, e_sm, e_data))
    assert np.isfinite(want_s).all() and np.isfinite(sm).all()
    assert e_orig < 1e-6
    assert e_sm < ATOL_SMOOTH
    assert e_data < ATOL_DATA


# ---- 4. one region per point; the point limit ----

def test_one_region_per_point_yields_the_original_cloud_and_2048_points_are_refused():
    data = _cloud(3, 64).to(DEV)
    rid = np.random.default_rng(1).permutation(64).astype(np.int64)
    poses, sm, res = smoothness.enumerate_smoothness(data, rid, enum_args("planarity", num_regions=64), "inc", wide=True)
    assert poses.shape == (1, 64, 3) and torch.equal(poses[0], data[0])
    assert np.all(res["stop_epoch_host"] == -1) and sm.shape == (1, 64) and np.isnan(sm).all()
    big = _cloud(3, 2048)[0].to(DEV).contiguous()
    with pytest.raises(_lib.IqError, match="N=2048"):
        hip_ops.smoothness_enum_wide(big, torch.zeros((2048,), dtype=torch.int32, device=DEV), 128, "planarity", "inc")
    with pytest.raises(_lib.IqError):
        hip_ops.smoothness_enum_wide(big[:1024].contiguous(), torch.zeros((1024,), dtype=torch.int32, device=DEV), 1025, "planarity", "inc")
    with pytest.raises(_lib.IqError):       # the narrow entry keeps its limit
        hip_ops.smoothness_enum(big[:1024].contiguous(), torch.zeros((1024,), dtype=torch.int32, device=DEV), 65, "planarity", "inc")


# ---- 5. the driver ----

def test_final_wide_smoothness_driver_end_to_end(tmp_path):
    wd.run_child([wd.step(tmp_path, "final_wide_shapley.py", wd.STAGE1), wd.step(tmp_path, "final_wide_smoothness.py", wd.POSE)])
    root = tmp_path / wd.EXP
    region_id, orders = np.load(root / "region_id.npy"), np.load(root / "all_orders.npy")
    pts, y = synth.make_cloud(0)
    data, lbl = torch.from_numpy(pts)[None].to(DEV), torch.tensor([y]).to(DEV)
    model, _ = probes.coalition_model("pointnet", DEV)
    args = argparse.Namespace(model="pointnet", softmax_type="modified", num_points=1024, num_regions=wd.REGIONS, verbose=False)
    _, _, total = wide.shapley(model, data, lbl, region_id, orders, args)
    for mode in hip_ops.SMOOTHNESS_MODES:
        for objective in ("inc", "dec"):
            folder = root / ("%s_all" % mode) / ("allregion_%s" % objective)
            phi, sm, clouds = np.load(folder / "region_shapley_value.npy"), np.load(folder / ("%s.npy" % mode)), np.load(folder / "data_smoothness.npy")
            p = phi.shape[0]
            assert 1 <= p <= smoothness.EPOCH and phi.shape == (p, wd.REGIONS) and phi.dtype == np.float64
            assert sm.shape == (p, wd.REGIONS) and sm.dtype == np.float64
            assert clouds.shape == (p, 1, 1024, 3) and clouds.dtype == np.float32
            assert np.array_equal(np.load(folder / "orig_shapley_value.npy"), total / wd.SAMPLES)
            assert (folder / "log.txt").exists() and not (folder / "all_logits.pt").exists()
            for e in {0, p - 1}:
                _, _, want = wide.shapley(model, torch.from_numpy(clouds[e]).to(DEV), lbl, region_id, orders, args)
                assert np.array_equal(phi[e], want / wd.SAMPLES)
        sens = ref_cpu.consumer_sensitivity(str(root) + "/", mode)
        assert sens.shape == (wd.REGIONS,) and np.isfinite(sens).all()
