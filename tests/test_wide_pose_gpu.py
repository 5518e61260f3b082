"""GPU: the pose sweeps of wide games (wide.shapley_over_poses, wide.sharded_shapley, final_wide_pose.py,
final_wide_interaction.py --adv_pose sweep).

The yardstick of every value is ``wide.shapley`` on the one pose - the code path that existed before the sweeps - bit for bit.
Other bars (none is new):
  * Shapley values against oracle.ref_cpu.shap_sampling_all_regions_batch on the perturbed cloud: 1e-4 norm-wise;
  * efficiency: sum(phi) against v(all) - v(none), R float32 roundings of at most 2 max|v| 2^-24 each (tests/test_wide_gpu.py);
  * one process against two ranks: every artefact file bitwise.
Shapes: N = 256 with R = 65 (two words per keep row) and R = 256 (one region per point, three 96-row chunks); S = 3 permutations,
P = 3 poses; with 300 coalitions to a launch a pose's permutations split over launches (R = 256).
"""
import argparse
import math
import os
import sys

import numpy as np
import pytest
import torch

import probes
import wide_drivers as wd
from interpret_quality_amd import _lib, final_common, hip_ops, pose_sweep, synth, wide
from oracle import ref_cpu
from test_dist_gpu import _artefacts, _assert_same, _env, _run_chains, _torchrun

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _args(family, num_regions, num_points):
    return argparse.Namespace(model=family, softmax_type="modified", num_points=num_points, num_regions=num_regions, verbose=False)


def _poses(data):
    """One rotation, one translation, one scale of ``data`` (1,N,3) on the device -> (3,N,3)."""
    return torch.cat([pose_sweep.rotate_xyz(data, torch.tensor([0.3, -0.5, 0.7], device=data.device)),
                      pose_sweep.translate_pc(data, torch.tensor([0.2, -0.1, 0.3], device=data.device)),
                      pose_sweep.scale_pc(data, torch.tensor(1.5, device=data.device))], dim=0).contiguous()


_CASES = {}


def _case(n, r, s=3):
    """PointNet on cloud 0 cut to n points: inputs, and per route the yardstick - wide.shapley on each pose (computed once)."""
    if (n, r) not in _CASES:
        pts, y = synth.make_cloud(0, n)
        data, lbl = torch.from_numpy(pts)[None], torch.tensor([y])
        if r == n:
            rid = np.random.default_rng(r).permutation(n).astype(np.int64)
        else:
            rid = np.asarray(ref_cpu.cal_region_id(data, ref_cpu.farthest_point_sample(data, r)[0].numpy())).astype(np.int64)
        orders = synth.make_orders(s, r, seed=7)
        model, sd = probes.coalition_model("pointnet", DEV)
        poses = _poses(data.to(DEV))
        args = _args("pointnet", r, n)
        want = {route: np.stack([wide.shapley(model, poses[p:p + 1], lbl.to(DEV), rid, orders, args, route=route)[2] / s
                                 for p in range(poses.shape[0])]) for route in wide.ROUTES}
        _CASES[(n, r)] = dict(data=data, lbl=lbl, rid=rid, orders=orders, model=model, sd=sd, poses=poses, args=args, want=want)
    return _CASES[(n, r)]


# ---- 1. PointNet: the bitwise contract ----

@pytest.mark.parametrize("route", wide.ROUTES)
@pytest.mark.parametrize("n,r", [(256, 65), (256, 256)])
def test_pointnet_poses_equal_wide_shapley_on_each_pose_bitwise(n, r, route, monkeypatch):
    c = _case(n, r)
    phi = wide.shapley_over_poses(c["model"], c["poses"], c["lbl"].to(DEV), c["rid"], c["orders"], c["args"], route=route)
    assert phi.shape == (3, r) and phi.dtype == torch.float64 and phi.is_cuda
    assert np.array_equal(phi.cpu().numpy(), c["want"][route])
    assert np.array_equal(c["want"]["prefix"], c["want"]["keep"])          # the routes give the same bits
    # 300 coalitions to a launch: at R = 256 every permutation is a launch of its own (the keep route: three launches a pose)
    monkeypatch.setattr(type(c["model"]), "max_wide_per_call", 300)
    split = wide.shapley_over_poses(c["model"], c["poses"], c["lbl"].to(DEV), c["rid"], c["orders"], c["args"], route=route)
    assert np.array_equal(split.cpu().numpy(), c["want"][route])


@pytest.mark.parametrize("n,r", [(256, 65), (256, 256)])
def test_pose_values_sum_to_v_full_minus_v_empty(n, r):
    c = _case(n, r)
    phi = wide.shapley_over_poses(c["model"], c["poses"], c["lbl"].to(DEV), c["rid"], c["orders"], c["args"]).cpu().numpy()
    for p in range(3):
        logits = wide.prefix_logits(c["model"], c["poses"][p:p + 1], c["rid"], c["orders"], c["args"])
        v = final_common.get_reward(logits, c["lbl"].to(DEV), c["args"]).cpu().numpy().astype(np.float64).reshape(3, r + 1)
        assert np.all(v[:, 0] == v[0, 0]) and np.all(v[:, -1] == v[0, -1])       # v(none) and v(all) of every permutation
        bound = r * 2 * float(np.abs(v).max()) * 2.0 ** -24
        gap = abs(math.fsum(list(phi[p]) + [-v[0, -1], v[0, 0]]))
        print("N=%d R=%d pose %d: efficiency gap / bound = %.3g" % (n, r, p, gap / bound))
        assert gap <= bound, (gap, bound)


# ---- 2. against the CPU oracle ----

def test_pose_values_match_the_oracle_on_the_perturbed_clouds():
    c = _case(256, 65)
    phi = wide.shapley_over_poses(c["model"], c["poses"], c["lbl"].to(DEV), c["rid"], c["orders"], c["args"]).cpu().numpy()
    oracle = ref_cpu.PointNetOracle(c["sd"])
    for p in range(3):
        want, _ = ref_cpu.shap_sampling_all_regions_batch(oracle, c["poses"][p:p + 1].cpu(), c["lbl"], c["rid"], c["orders"], 3, 3, 65)
        err = float(np.linalg.norm(phi[p] - want) / np.linalg.norm(want))
        print("pose %d vs oracle: rel %.3g" % (p, err))
        assert err <= 1e-4


# ---- 3. the other families ----

@pytest.mark.parametrize("coalitions", [None, "compact"])
@pytest.mark.parametrize("family", ["gcnn", "pointnet2"])
def test_other_families_equal_wide_shapley_on_each_pose_bitwise(family, coalitions):
    n, r, s = 128, 65, 2
    model, _ = probes.coalition_model(family, DEV)
    pts, y = synth.make_cloud(0, n)
    data, lbl = torch.from_numpy(pts)[None].to(DEV), torch.tensor([y]).to(DEV)
    rid = np.random.default_rng(13).integers(0, r, size=n)
    rid[:r] = np.arange(r)
    orders = synth.make_orders(s, r, seed=5)
    args = _args(family, r, n)
    poses = _poses(data)[:2].contiguous()
    phi = wide.shapley_over_poses(model, poses, lbl, rid, orders, args, coalitions=coalitions).cpu().numpy()
    assert phi.shape == (2, r) and np.isfinite(phi).all()
    for p in range(2):
        _, _, total = wide.shapley(model, poses[p:p + 1], lbl, rid, orders, args, coalitions=coalitions)
        assert np.array_equal(phi[p], total / s)


# ---- 4. error paths ----

def test_error_paths():
    c = _case(256, 65)
    lbl = c["lbl"].to(DEV)
    gcnn, _ = probes.coalition_model("gcnn", DEV)
    with pytest.raises(_lib.IqError, match="prefix"):
        wide.shapley_over_poses(gcnn, c["poses"], lbl, c["rid"], c["orders"], _args("gcnn", 65, 256), route="prefix")
    with pytest.raises(_lib.IqError, match="orders"):
        wide.shapley_over_poses(c["model"], c["poses"], lbl, c["rid"], c["orders"][:, :64], c["args"])
    empty = wide.shapley_over_poses(c["model"], c["poses"][:0], lbl, c["rid"], c["orders"], c["args"])
    assert empty.shape == (0, 65) and empty.dtype == torch.float64
    # the original cloud travels as pose 0 of the sharded call; a single process holds every pose
    orig, phi = wide.sharded_shapley(c["model"], c["data"].to(DEV), c["poses"], lbl, c["rid"], c["orders"], c["args"])
    _, _, total = wide.shapley(c["model"], c["data"].to(DEV), lbl, c["rid"], c["orders"], c["args"])
    assert orig.shape == (65,) and np.array_equal(orig, total / 3) and np.array_equal(phi.cpu().numpy(), c["want"]["prefix"])


# ---- 5. the drivers, in one child process ----

def test_wide_pose_and_adversarial_interaction_drivers_end_to_end(tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir()
    adv_file = str(a / wd.EXP / "interaction_seed1" / "rotate_adv" / "transform_params.npy")
    inter = wd.COMMON + ["--mode", "rotate", "--num_pairs_random", "3", "--num_save_context_max", "2"]
    wd.run_child([wd.step(a, "final_wide_shapley.py", wd.STAGE1),
                  wd.step(a, "final_wide_pose.py", wd.POSE + ["--mode", "scale"]),
                  wd.step(a, "final_wide_pose.py", wd.POSE + ["--mode", "rotate"]),
                  {"copytree": [str(a), str(b)]},
                  wd.step(a, "final_wide_interaction.py", inter + ["--adv_pose", "sweep"]),
                  wd.step(b, "final_wide_interaction.py", inter + ["--transform_params", adv_file])])
    root = a / wd.EXP
    region_id, orders = np.load(root / "region_id.npy"), np.load(root / "all_orders.npy")
    assert orders.shape == (wd.SAMPLES, wd.REGIONS)
    data, lbl = torch.from_numpy(synth.make_cloud(0)[0])[None].to(DEV), torch.tensor([synth.make_cloud(0)[1]]).to(DEV)
    model, _ = probes.coalition_model("pointnet", DEV)
    args = _args("pointnet", wd.REGIONS, 1024)
    _, _, total = wide.shapley(model, data, lbl, region_id, orders, args)
    for mode, n_pose, files, disturb in (("scale", 30, {"scale.npy": (30,)}, pose_sweep.scale_pc),
                                         ("rotate", 216, {"angle_tuple.npy": (216, 3)}, pose_sweep.rotate_xyz)):
        folder = root / ("%s_all" % mode)
        phi = np.load(folder / "region_shapley_value.npy")
        assert phi.shape == (n_pose, wd.REGIONS) and phi.dtype == np.float64
        assert np.array_equal(np.load(folder / "orig_shapley_value.npy"), total / wd.SAMPLES)
        for name, shape in files.items():
            assert np.load(folder / name).shape == shape
        assert (folder / "log.txt").exists() and not (folder / "all_logits.pt").exists()
        params = torch.from_numpy(np.load(folder / list(files)[0])).to(DEV)
        for k in (1, n_pose - 1):
            _, _, want = wide.shapley(model, disturb(data, params[k]), lbl, region_id, orders, args)
            assert np.array_equal(phi[k], want / wd.SAMPLES)
    sens = ref_cpu.consumer_sensitivity(str(root) + "/", "scale")
    assert sens.shape == (wd.REGIONS,) and np.isfinite(sens).all() and np.all(sens >= 0)
    # --adv_pose sweep: the pose with the lowest reward on the true class, by one dense forward over the 216 poses
    angles = np.load(root / "rotate_all" / "angle_tuple.npy")
    poses = torch.cat([pose_sweep.rotate_xyz(data, torch.from_numpy(angles[i]).to(DEV)) for i in range(216)], dim=0)
    v = final_common.get_reward(model(poses.permute(0, 2, 1).contiguous())[0], lbl, args)
    adv = root / "interaction_seed1" / "rotate_adv"
    pose_idx = np.load(adv / "pose_idx.npy")
    assert pose_idx.shape == () and int(pose_idx) == int(torch.argmin(v).item())
    assert np.array_equal(np.load(adv / "transform_params.npy"), angles[int(pose_idx)])
    # ... evaluated exactly as --transform_params with that row
    other = b / wd.EXP / "interaction_seed1" / "rotate_adv"
    names = sorted(f for f in os.listdir(adv) if f != "pose_idx.npy")
    assert names == sorted(os.listdir(other)) and any(f.endswith("_interaction.npy") for f in names)
    for f in names:
        if f.endswith(".npy"):
            assert np.array_equal(np.load(adv / f), np.load(other / f), equal_nan=True), f
        elif f.endswith(".pt"):
            assert torch.equal(torch.load(adv / f, map_location="cpu"), torch.load(other / f, map_location="cpu")), f
        else:
            assert open(adv / f).read() == open(other / f).read(), f


# ---- 6. two ranks ----

def test_two_ranks_write_the_same_pose_and_smoothness_artefacts_as_one_process(tmp_path):
    """The wide pose sweep (poses sharded) and the wide smoothness stage (epochs sharded) under the two-rank rehearsal of
    tests/test_dist_gpu.py against one process, each in its own directory: every artefact file bitwise identical."""
    plan = [("final_wide_shapley.py", wd.STAGE1), ("final_wide_pose.py", wd.POSE + ["--mode", "scale"]), ("final_wide_smoothness.py", wd.POSE)]
    chains = []
    for tag in ("one", "two"):     # side by side: three processes on the card
        work = tmp_path / tag
        work.mkdir()
        chains.append([(([sys.executable] if tag == "one" else _torchrun(2, 29721 + k)) + [os.path.join(wd.REPO, script)] + extra, work,
                        _env(IQ_REHEARSAL="1") if tag == "two" else _env()) for k, (script, extra) in enumerate(plan)])
    _run_chains(chains)
    one, two = _artefacts(tmp_path / "one"), _artefacts(tmp_path / "two")
    assert any(k.endswith(os.path.join("scale_all", "region_shapley_value.npy")) for k in one)
    assert any(k.endswith(os.path.join("planarity_all", "allregion_dec", "data_smoothness.npy")) for k in one)
    _assert_same(one, two)
