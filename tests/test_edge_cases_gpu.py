"""GPU: edge cases of the hot path - empty / full / single-region coalitions, empty regions, the maximum
region count, smaller clouds, empty batches, and the error behaviour of the C ABI."""
import ctypes

import numpy as np
import pytest
import torch

from interpret_quality_amd import _lib, hip_ops, synth
from interpret_quality_amd.pointnet import PointNetCls

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def model(pointnet_sd):
    m = PointNetCls(None)
    m.load_state_dict(pointnet_sd)
    return m.to(dev()).eval()


@pytest.fixture(scope="module")
def oracle_model(pointnet_sd):
    from oracle import ref_cpu
    return ref_cpu.PointNetOracle(pointnet_sd)


def masked_by_keep(pts, region_id, keep, center):
    out = np.repeat(pts[None], len(keep), axis=0).copy()
    for b, k in enumerate(keep):
        drop = ((np.uint64(k) >> np.asarray(region_id).astype(np.uint64)) & np.uint64(1)) == 0
        out[b, drop] = center
    return out


def check_against_oracle(model, oracle_model, pts, region_id, num_regions, keep):
    d = dev()
    data = torch.from_numpy(pts).unsqueeze(0)
    center = torch.mean(data, dim=1)
    got = model.coalition_logits(data.to(d), center.to(d), hip_ops.as_i32(region_id, d).reshape(1, -1),
                                 hip_ops.masks_to_tensor(keep, d), None, num_regions=num_regions).cpu().numpy()
    x = torch.from_numpy(masked_by_keep(pts, region_id, keep, center[0].numpy())).permute(0, 2, 1).contiguous()
    want = oracle_model(x)[0].numpy()
    assert np.abs(got - want).max() / np.abs(want).max() < 1e-4


def test_extreme_coalitions_and_max_region_count(model, oracle_model):
    pts, _ = synth.make_cloud(5)
    rng = np.random.default_rng(0)
    region_id = rng.integers(0, 64, size=1024)            # R = 64: the ABI maximum (uint64 masks)
    keep = [0, (1 << 64) - 1, 1, 1 << 63, (1 << 64) - 2, 0x5555555555555555, 1 << 17]
    check_against_oracle(model, oracle_model, pts, region_id, 64, keep)


def test_empty_regions_and_single_region(model, oracle_model):
    pts, _ = synth.make_cloud(6)
    region_id = np.zeros(1024, dtype=np.int64)
    region_id[:100] = 5                                   # regions 1-4, 6, 7 are empty
    # keeping only empty regions masks everything; dropping only empty regions masks nothing (no centre row)
    check_against_oracle(model, oracle_model, pts, region_id, 8, [0, 0b11011110, 0b00100001, 0b1, 0b100000, 0xff])
    check_against_oracle(model, oracle_model, pts, np.zeros(1024, dtype=np.int64), 1, [0, 1])   # R = 1


def test_smaller_cloud_and_batch_of_one(model, oracle_model):
    pts, _ = synth.make_cloud(7, num_points=512)          # N = 512 (< the 1024 of the reference)
    rng = np.random.default_rng(1)
    check_against_oracle(model, oracle_model, pts, rng.integers(0, 32, size=512), 32, [0x0f0f0f0f])


def test_empty_batches_everywhere(model):
    d = dev()
    cloud = torch.zeros((1, 1024, 3), device=d)
    rid = torch.zeros((1, 1024), dtype=torch.int32, device=d)
    out = model.coalition_logits(cloud, torch.zeros((1, 3), device=d), rid, torch.zeros((0,), dtype=torch.int64, device=d),
                                 None, num_regions=32)
    assert tuple(out.shape) == (0, 10)
    assert hip_ops.reward(torch.zeros((0, 10), device=d), 0).shape == (0,)
    phi, rows, _ = hip_ops.shapley_accum(torch.zeros((0,), device=d), torch.zeros((0, 32), dtype=torch.int32, device=d))
    assert phi.shape == (32,) and float(phi.abs().sum()) == 0.0 and rows.shape == (0, 32)
    assert hip_ops.interaction_reduce(torch.zeros((0,), device=d)).shape == (0,)
    assert hip_ops.mask_interaction(cloud[0], rid[0], torch.zeros((0, 2), dtype=torch.int32, device=d),
                                    torch.zeros((0,), dtype=torch.int64, device=d), torch.zeros(3, device=d), 32).shape == (0, 3, 1024)


def test_abi_error_reporting(model):
    lib = _lib.load()
    d = dev()
    # unsupported sizes -> negative code + message, nothing is launched
    cloud = torch.zeros((4100, 3), device=d)
    with pytest.raises(_lib.IqError, match="not in"):
        hip_ops.mask_shapley(cloud, torch.zeros(4100, dtype=torch.int32, device=d), torch.zeros((1, 8), dtype=torch.int32, device=d),
                             torch.zeros(3, device=d))
    with pytest.raises(_lib.IqError, match="label"):
        hip_ops.reward(torch.zeros((4, 10), device=d), 10)
    # workspace too small -> IQ_EWORKSPACE
    eng = model.engine()
    clouds = torch.zeros((1, 1024, 3), device=d)
    rid = torch.zeros((1, 1024), dtype=torch.int32, device=d)
    keep = torch.zeros((4,), dtype=torch.int64, device=d)
    logits = torch.empty((4, 10), device=d)
    tiny = torch.empty(1024, dtype=torch.uint8, device=d)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = lib.iq_pointnet_coalitions(ctypes.byref(eng.weights.struct), p(clouds), p(torch.zeros((1, 3), device=d)), p(rid),
                                    p(keep), None, p(logits), None, p(tiny), tiny.numel(), 4, 1, 1024, 32, 0, None)
    assert rc == -3 and b"workspace" in lib.iq_last_error()
    # N beyond the fused kernel's row-list capacity
    rc = lib.iq_pointnet_coalitions(ctypes.byref(eng.weights.struct), p(clouds), None, p(rid), None, None, p(logits), None,
                                    p(tiny), tiny.numel(), 1, 1, 4097, 1, 0, None)
    assert rc == -1 and b"N=4097" in lib.iq_last_error()
    # wrong dtype / device at the Python boundary
    with pytest.raises(_lib.IqError):
        hip_ops.fps(torch.zeros((1, 64, 3), dtype=torch.float64, device=d), 8)
    with pytest.raises(_lib.IqError):
        model.coalition_logits(clouds.cpu(), None, rid, None, None, num_regions=1)


@pytest.mark.parametrize("accum", [hip_ops.shapley_accum, hip_ops.shapley_accum_wide])
def test_shapley_accum_refuses_a_reward_vector_of_the_wrong_length(accum):
    """S = 2 permutations of R = 3 regions need 8 rewards: one short would be read out of bounds, so nothing is launched."""
    d = dev()
    orders = torch.tensor([[0, 1, 2], [2, 0, 1]], dtype=torch.int32, device=d)
    v = torch.arange(8, dtype=torch.float32, device=d)
    with pytest.raises(_lib.IqError, match="v holds 7 rewards for 2 permutations of 3 regions"):
        accum(v[:7].contiguous(), orders, snap_counts=[1])
    phi, rows, snaps = accum(v, orders, snap_counts=[1])
    assert rows.shape == (2, 3) and torch.equal(phi, rows.sum(0)) and torch.equal(snaps[0], rows[0])
    assert rows[0].tolist() == [1.0, 1.0, 1.0] and rows[1].tolist() == [1.0, 1.0, 1.0]      # v[i+1] - v[i], credited to orders[o][i]


def test_fps_more_samples_than_distinct_points():
    d = dev()
    x = torch.zeros((2, 64, 3), device=d)
    x[0, 10, 0] = 1.0
    x[0, 20, 1] = 2.0
    got = hip_ops.fps(x, 8).cpu().numpy()
    assert got[0].tolist() == [0, 20, 10, 0, 0, 0, 0, 0]      # farthest first, then index 0 forever
    assert got[1].tolist() == [0] * 8


def _degenerate_clouds():
    """(4,1024,3): everything masked (one distinct location), one region of 32 kept, all but one kept, raw."""
    from oracle import ref_cpu as O
    pts, _ = synth.make_cloud(8)
    data = torch.from_numpy(pts).unsqueeze(0)
    rid = O.cal_region_id(data, O.farthest_point_sample(data, 32)[0])
    center = torch.mean(data, dim=1)[0].numpy()
    keep = [0, 1 << 3, ((1 << 32) - 1) ^ (1 << 9), (1 << 32) - 1]
    return torch.from_numpy(masked_by_keep(pts, np.asarray(rid), keep, center)).permute(0, 2, 1).contiguous()


@pytest.mark.parametrize("name", ["pointnet2", "dgcnn", "gcnn", "pointconv"])
def test_degenerate_clouds_other_models(name):
    import argparse
    from oracle import ref_cpu as O
    from interpret_quality_amd.dgcnn import DGCNN_cls, GCNN_cls
    from interpret_quality_amd.pointconv import PointConvDensityClsSsg
    from interpret_quality_amd.pointnet2 import PointNet2ClsMsg
    ns = argparse.Namespace(dataset="modelnet10", k=20)
    cls, sd, orc = {
        "pointnet2": (PointNet2ClsMsg, synth.pointnet2_state_dict, O.PointNet2Oracle),
        "dgcnn": (DGCNN_cls, synth.dgcnn_state_dict, lambda s: O.DgcnnOracle(s, k=20, fixed_graph=False)),
        "gcnn": (GCNN_cls, synth.dgcnn_state_dict, lambda s: O.DgcnnOracle(s, k=20, fixed_graph=True)),
        "pointconv": (PointConvDensityClsSsg, synth.pointconv_state_dict, O.PointConvOracle),
    }[name]
    sd = synth.to_torch(sd(0))
    m = cls(ns if "cnn" in name else None)
    m.load_state_dict(sd)
    m = m.to(dev()).eval()
    x = _degenerate_clouds()
    got = m(x.to(dev()))
    got = (got[0] if isinstance(got, tuple) else got).cpu().numpy()
    want = orc(sd)(x)
    want = (want[0] if isinstance(want, tuple) else want).numpy()
    assert np.isfinite(got).all()
    if name == "dgcnn":
        # DGCNN's feature-space graphs: on two of these clouds a query sits on a kNN near-tie and the reference's float32 run
        # decides it differently from its OWN float64 run (logits move by 1e-3 and 2e-3).  The HIP path re-ranks near-ties in
        # exact arithmetic (knn_refine_kernel), so the yardstick is the ORACLE RUN IN DOUBLE (the reference itself cannot travel to
        # this box; the oracle in double is pinned against the reference's float64 logits by
        # tests/test_oracle_golden.py::test_oracle_dgcnn_fp64_on_a_slice_of_the_scale_fixture), and wherever the float32 oracle
        # agrees with its double run, so does the HIP path with the float32 oracle.
        sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
        want64 = orc(sd64)(x.double()).numpy()
        scale = np.abs(want).max()
        assert np.abs(got - want64).max() / scale < 1e-4
        settled = np.abs(want - want64).max(axis=1) / scale < 1e-5            # clouds on which the reference agrees with itself
        assert settled.sum() >= 2 and np.abs(got - want)[settled].max() / scale < 1e-4
        return
    assert np.abs(got - want).max() / np.abs(want).max() < 1e-4


def test_shapenet_loader_downsamples_on_the_hip_path(tmp_path, monkeypatch):
    """final_data_shapley.py:95-179: loadtxt -> centre -> scale -> FPS(1024) -> gather, items bit-identical to the
    reference's (its NumPy sampler is iq_fps here), plus the raw sampler on a 2607-point scan."""
    import argparse
    from conftest import load_golden
    from interpret_quality_amd import data_shapley, final_util
    g = load_golden("loaders.npz")
    raw = synth.raw_scan(10, 2607).astype(np.float32)
    assert np.array_equal(data_shapley.farthest_point_sample_np(raw, 64), g["fps_np_2607_to_64"])
    synth.write_dataset_tree(str(tmp_path))
    monkeypatch.chdir(tmp_path)
    args = argparse.Namespace(dataset="shapenet", num_points=1024, device=dev())
    ds = data_shapley.ShapeNetDataset_Shapley_test(args, split="train", npoints=1024,
                                                   class_choice=final_util.SHAPENET_CLASS, classification=True)
    assert len(ds) == int(g["shapenet_len"])
    for i in range(len(ds)):
        pts, cls = ds[i]
        assert pts.dtype == torch.float32 and cls.dtype == torch.int64 and cls.dim() == 0
        assert np.array_equal(pts.numpy(), g["shapenet_%d_points" % i])
        assert int(cls) == int(g["shapenet_%d_label" % i])
    batches = list(data_shapley.shapley_test_loader(args))
    assert len(batches) == 3 and tuple(batches[0][0].shape) == (1, 1024, 3) and tuple(batches[0][1].shape) == (1,)
    with pytest.raises(_lib.IqError, match="exceeds"):
        data_shapley.farthest_point_sample_np(np.zeros((9000, 3), dtype=np.float32), 8)


@pytest.mark.parametrize("name", ["pointnet2", "dgcnn", "gcnn"])
def test_coalition_paths_on_smaller_clouds_and_max_regions(name):
    """The coalition entry points of PointNet++ (pair tables) and DGCNN / GCNN (compact clouds) on 512-point clouds
    with 64 regions, against the same model's forward on the materialised clouds."""
    import argparse
    from interpret_quality_amd.dgcnn import DGCNN_cls, GCNN_cls
    from interpret_quality_amd.pointnet2 import PointNet2ClsMsg
    cls, sd = {"pointnet2": (PointNet2ClsMsg, synth.pointnet2_state_dict), "dgcnn": (DGCNN_cls, synth.dgcnn_state_dict),
               "gcnn": (GCNN_cls, synth.dgcnn_state_dict)}[name]
    m = cls(argparse.Namespace(dataset="modelnet10", k=20) if "cnn" in name else None)
    m.load_state_dict(synth.to_torch(sd(0)))
    m = m.to(dev()).eval()
    d = dev()
    pts, _ = synth.make_cloud(9, num_points=512)
    cloud = torch.from_numpy(pts).unsqueeze(0).to(d)
    rng = np.random.default_rng(2)
    rid = torch.from_numpy(rng.integers(0, 64, size=(1, 512)).astype(np.int32)).to(d)
    center = cloud.mean(dim=1)
    keep = [(1 << 64) - 1, 0, 0x00ff00ff00ff00ff, 1 << 63, (1 << 64) - 2]
    got = m.coalition_logits(cloud, center, rid, hip_ops.masks_to_tensor(keep, d), None, num_regions=64)
    dense = hip_ops.mask_coalitions(cloud[0], rid[0].contiguous(), hip_ops.masks_to_tensor(keep, d), center[0].contiguous())
    want = m.forward_points(dense)
    assert np.isfinite(got.cpu().numpy()).all()
    assert np.abs((got - want).cpu().numpy()).max() / np.abs(want.cpu().numpy()).max() < 1e-5


def test_abi_error_reporting_of_the_coalition_and_enumeration_entry_points():
    import argparse
    from interpret_quality_amd.dgcnn import DGCNN_cls
    from interpret_quality_amd.pointnet2 import PointNet2ClsMsg
    lib = _lib.load()
    d = dev()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    clouds = torch.zeros((1, 1024, 3), device=d)
    centers = torch.zeros((1, 3), device=d)
    rid = torch.zeros((1, 1024), dtype=torch.int32, device=d)
    keep = torch.zeros((4,), dtype=torch.int64, device=d)
    logits = torch.empty((4, 10), device=d)
    tiny = torch.empty(4096, dtype=torch.uint8, device=d)
    dg = DGCNN_cls(argparse.Namespace(dataset="modelnet10", k=20))
    dg.load_state_dict(synth.to_torch(synth.dgcnn_state_dict(0)))
    eng = dg.to(d).eval().engine()
    args = (ctypes.byref(eng.weights.struct), p(clouds), p(centers), p(rid), p(keep), None, p(logits), p(tiny), tiny.numel())
    assert lib.iq_dgcnn_coalitions(*args, 4, 1, 1024, 0, None) == -3 and b"workspace" in lib.iq_last_error()
    assert lib.iq_dgcnn_coalitions(*args, 4, 1, 10, 0, None) == -1 and b"N=10" in lib.iq_last_error()   # fewer points than k
    assert lib.iq_dgcnn_coalitions(*args, 4, 3, 1024, 0, None) == -1 and b"cloud_of" in lib.iq_last_error()
    assert lib.iq_dgcnn_coalitions(*args, 0, 1, 1024, 0, None) == 0                       # empty batch: nothing to do
    pn = PointNet2ClsMsg(None)
    pn.load_state_dict(synth.to_torch(synth.pointnet2_state_dict(0)))
    e2 = pn.to(d).eval().engine()
    args2 = (ctypes.byref(e2.weights.struct), p(clouds), p(centers), p(rid), p(keep), None, p(logits), p(tiny), tiny.numel())
    assert lib.iq_pointnet2_coalitions(*args2, 4, 1, 1024, None) == -3 and b"workspace" in lib.iq_last_error()
    assert lib.iq_pointnet2_coalitions(*args2, 4, 0, 1024, None) == -1
    assert lib.iq_pointnet2_coalitions_workspace_bytes(4, 1, 1024) > lib.iq_pointnet2_workspace_bytes(4)
    with pytest.raises(_lib.IqError, match="N=2048"):
        hip_ops.smoothness_enum(torch.zeros((2048, 3), device=d), torch.zeros(2048, dtype=torch.int32, device=d), 4, "linearity", "inc")
    with pytest.raises(_lib.IqError, match="mode"):
        hip_ops.smoothness_enum(torch.zeros((64, 3), device=d), torch.zeros(64, dtype=torch.int32, device=d), 4, "roundness", "inc")
    with pytest.raises(_lib.IqError):
        hip_ops.linear(torch.zeros((4, 12), device=d), hip_ops.PackedLinear(np.zeros((8, 16), np.float32), np.zeros(8, np.float32), d))


@pytest.mark.parametrize("name", ["pointnet", "pointnet2", "dgcnn", "gcnn", "pointconv"])
def test_a_coalitions_logits_do_not_depend_on_the_batch_it_travels_in(name):
    """Bitwise: logits of coalitions 10..24 evaluated alone equal rows 10..24 of the 40-coalition launch.  (Sharding over
    ranks and the drivers' batching rely on this; a row-count-dependent split-K once broke it for PointConv.)"""
    import argparse
    from interpret_quality_amd import final_common
    from interpret_quality_amd.dgcnn import DGCNN_cls, GCNN_cls
    from interpret_quality_amd.pointconv import PointConvDensityClsSsg
    from interpret_quality_amd.pointnet2 import PointNet2ClsMsg
    cls, sd = {"pointnet": (PointNetCls, synth.pointnet_state_dict), "pointnet2": (PointNet2ClsMsg, synth.pointnet2_state_dict),
               "dgcnn": (DGCNN_cls, synth.dgcnn_state_dict), "gcnn": (GCNN_cls, synth.dgcnn_state_dict),
               "pointconv": (PointConvDensityClsSsg, synth.pointconv_state_dict)}[name]
    m = cls(argparse.Namespace(dataset="modelnet10", k=20) if "cnn" in name else None)
    m.load_state_dict(synth.to_torch(sd(0)))
    m = m.to(dev()).eval()
    d = dev()
    pts, _ = synth.make_cloud(11)
    cloud = torch.from_numpy(pts).unsqueeze(0).to(d)
    rid = hip_ops.region_assign(cloud[0].contiguous(), hip_ops.fps(cloud, 32)[0].contiguous()).reshape(1, -1)
    center = cloud.mean(dim=1)
    rng = np.random.default_rng(4)
    keep = [int(x) for x in rng.integers(0, 1 << 32, size=40)]

    def logits(ks):
        kt = hip_ops.masks_to_tensor(ks, d)
        if hasattr(m, "coalition_logits"):
            return m.coalition_logits(cloud, center, rid, kt, None, num_regions=32)
        return m.forward_points(hip_ops.mask_coalitions(cloud[0], rid[0].contiguous(), kt, center[0].contiguous()))
    full = logits(keep)
    assert torch.equal(logits(keep[10:25]), full[10:25])
    assert torch.equal(logits(keep[39:]), full[39:])


@pytest.mark.parametrize("n", [100, 1000, 2500, 4096])      # (beyond 1024 points since round 5: the row lists hold up to IQ_MAX_POINTS)
def test_pointnet_coalitions_on_odd_cloud_sizes(model, oracle_model, n):
    """N that is not a multiple of the 64-row chunk / 32-row MFMA tile (the reference accepts any N)."""
    pts, _ = synth.make_cloud(12, num_points=n)
    rng = np.random.default_rng(n)
    check_against_oracle(model, oracle_model, pts, rng.integers(0, 16, size=n), 16, [0, 0xffff, 0x00ff, 0x8001, 0x5a5a])


@pytest.mark.parametrize("name", ["dgcnn", "gcnn"])
def test_graph_models_on_a_cloud_size_that_is_not_a_multiple_of_32(name):
    """N = 1000: dense forward against the oracle, and the coalition path against the dense forward (clouds are padded to
    a multiple of 32 with dead rows internally; the reference accepts any N >= k)."""
    import argparse
    from oracle import ref_cpu as O
    from interpret_quality_amd.dgcnn import DGCNN_cls, GCNN_cls
    sd = synth.to_torch(synth.dgcnn_state_dict(0))
    m = (DGCNN_cls if name == "dgcnn" else GCNN_cls)(argparse.Namespace(dataset="modelnet10", k=20))
    m.load_state_dict(sd)
    m = m.to(dev()).eval()
    d = dev()
    pts, _ = synth.make_cloud(13, num_points=1000)
    x = torch.from_numpy(pts).unsqueeze(0)
    want = O.DgcnnOracle(sd, k=20, fixed_graph=(name == "gcnn"))(x.permute(0, 2, 1).contiguous()).numpy()
    got = m(x.permute(0, 2, 1).contiguous().to(d)).cpu().numpy()
    assert np.abs(got - want).max() / np.abs(want).max() < 1e-4
    rid = torch.from_numpy(np.random.default_rng(0).integers(0, 8, size=(1, 1000)).astype(np.int32)).to(d)
    keep = [0xff, 0x0f, 0x00, 0x81]
    cloud, center = x.to(d), x.to(d).mean(dim=1)
    co = m.coalition_logits(cloud, center, rid, hip_ops.masks_to_tensor(keep, d), None, num_regions=8)
    dense = m.forward_points(hip_ops.mask_coalitions(cloud[0], rid[0].contiguous(), hip_ops.masks_to_tensor(keep, d), center[0].contiguous()))
    assert np.abs((co - dense).cpu().numpy()).max() / np.abs(dense.cpu().numpy()).max() < 1e-5


@pytest.mark.parametrize("name", ["pointnet2", "pointconv"])
def test_set_abstraction_models_on_a_cloud_size_that_is_not_a_multiple_of_32(name):
    from oracle import ref_cpu as O
    from interpret_quality_amd.pointconv import PointConvDensityClsSsg
    from interpret_quality_amd.pointnet2 import PointNet2ClsMsg
    cls, sdf, orc = {"pointnet2": (PointNet2ClsMsg, synth.pointnet2_state_dict, O.PointNet2Oracle),
                     "pointconv": (PointConvDensityClsSsg, synth.pointconv_state_dict, O.PointConvOracle)}[name]
    sd = synth.to_torch(sdf(0))
    m = cls(None)
    m.load_state_dict(sd)
    m = m.to(dev()).eval()
    pts, _ = synth.make_cloud(14, num_points=1000)
    x = torch.from_numpy(pts).unsqueeze(0).permute(0, 2, 1).contiguous()
    want = orc(sd)(x)
    want = (want[0] if isinstance(want, tuple) else want).numpy()
    got = m(x.to(dev()))
    got = (got[0] if isinstance(got, tuple) else got).cpu().numpy()
    assert np.abs(got - want).max() / np.abs(want).max() < 1e-4


def test_out_of_range_region_ids_and_orders_are_rejected_and_never_fault(model):
    """an id >= R or < 0 (a stale region_id.npy, a wrong num_regions) used to index LDS / the workspace out of
    bounds.  Now (a) iq_check_index_range names the first bad position, (b) every Python entry point that takes ids runs it
    (or its host twin), (c) the kernels themselves treat such a point as belonging to no region: no fault, finite output."""
    lib = _lib.load()
    d = dev()
    pts, _ = synth.make_cloud(2)
    data = torch.from_numpy(pts).unsqueeze(0).to(d)
    center = torch.mean(data, dim=1)
    rid = hip_ops.region_assign(data[0].contiguous(), hip_ops.fps(data, 8)[0].contiguous())
    hip_ops.check_index_range(rid, 0, 8, "region_id")                      # valid
    bad = rid.clone()
    bad[517] = 8
    bad[900] = -3
    with pytest.raises(_lib.IqError, match="position 517"):
        hip_ops.check_index_range(bad, 0, 8, "region_id")
    keep = hip_ops.masks_to_tensor([0, 0x0f, 0xff], d)
    for m_name in ("pointnet",):
        with pytest.raises(_lib.IqError, match="position 517"):
            model.coalition_logits(data, center, bad.reshape(1, -1), keep, None, num_regions=8)
    # the raw ABI with the same ids: no fault; the two bad points count as masked in every coalition
    got = model.coalition_logits(data, center, bad.reshape(1, -1), keep, None, num_regions=8, validate=False)
    torch.cuda.synchronize()
    assert torch.isfinite(got).all()
    pts2 = pts.copy()
    pts2[[517, 900]] = center[0].cpu().numpy()                              # = those two points moved onto the centre
    ok_rid = rid.clone()
    want = model.coalition_logits(torch.from_numpy(pts2).unsqueeze(0).to(d), center, ok_rid.reshape(1, -1), keep[:2].contiguous(),
                                  None, num_regions=8)
    assert torch.allclose(got[:2], want, rtol=1e-4, atol=1e-5)              # coalitions that mask something: same clouds
    # host-side twins used by the drivers for ids read from files
    with pytest.raises(_lib.IqError, match="region_id"):
        hip_ops.region_ids(bad.cpu().numpy().astype(np.int64), d, 8)
    from interpret_quality_amd import final_common, interaction
    with pytest.raises(_lib.IqError, match="orders"):
        final_common.prefix_keep_masks(np.array([[0, 1, 9]]), 8)
    with pytest.raises(_lib.IqError, match="region_pair_list"):
        interaction.context_keep_masks(np.array([[0, 8]]), np.zeros((1, 1, 0), dtype=np.int64), 8)
    # mask kernels and the accumulation with bad entries: defined, in-bounds
    orders = torch.tensor([[0, 1, 2, 3, 4, 5, 6, 77]], dtype=torch.int32, device=d)
    out = hip_ops.mask_shapley(data[0].contiguous(), bad, orders, center.reshape(3).contiguous())
    v = torch.arange(9, dtype=torch.float32, device=d)
    phi, rows, _ = hip_ops.shapley_accum(v, orders)
    torch.cuda.synchronize()
    assert torch.isfinite(out).all() and float(phi.sum().item()) == 7.0    # the 8th difference has nowhere to go


@pytest.mark.parametrize("n", [4096, 8192])
def test_fps_at_the_advertised_maximum_cloud_size(n):
    """iq_fps accepts N <= 8192 (16 N bytes of dynamic LDS: 64 KB at 4096, 128 KB at 8192 - above the default limit, so the
    launch opts in).  Checked against the oracle on a 2-cloud batch."""
    from oracle import ref_cpu as O
    rng = np.random.default_rng(n)
    x = rng.standard_normal((2, n, 3)).astype(np.float32)
    got = hip_ops.fps(torch.from_numpy(x).to(dev()), 64).cpu().numpy()
    want = O.farthest_point_sample(torch.from_numpy(x), 64).numpy()
    assert np.array_equal(got, want)


@pytest.mark.parametrize("n,s", [(1024, 512), (512, 128), (100, 32), (1000, 64)])
def test_fps_wave_per_cloud_kernel_equals_the_workgroup_kernel(n, s):
    """iq_fps picks its kernel by the batch: >= 64 clouds of <= 1024 points run one WAVE per cloud with the points in registers,
    smaller batches one workgroup per cloud through LDS.  Same picks on raw clouds, on masked clouds (FPS runs out of distinct
    locations and returns index 0 from then on) and on a fully collapsed cloud; a few clouds also against the oracle."""
    from oracle import ref_cpu as O
    rng = np.random.default_rng(n + s)
    clouds = []
    for i in range(72):
        pts = synth.make_cloud(i, 1024)[0][:n].copy()
        if i % 3 == 1:                                    # masked: a random subset collapses onto the centre
            drop = rng.random(n) < rng.uniform(0.3, 0.95)
            pts[drop] = pts.mean(axis=0)
        if i == 5:
            pts[:] = pts[0]                               # one location only
        clouds.append(pts)
    x = torch.from_numpy(np.stack(clouds)).to(dev())
    wave = hip_ops.fps(x, s).cpu().numpy()                                                 # 72 clouds: wave kernel
    block = np.concatenate([hip_ops.fps(x[i:i + 8].contiguous(), s).cpu().numpy() for i in range(0, 72, 8)])   # 8 at a time: workgroup kernel
    assert np.array_equal(wave, block)
    want = O.farthest_point_sample(x[:7].cpu(), s).numpy()
    assert np.array_equal(wave[:7], want)


def test_crt_points_of_coalitions_point_at_kept_points_or_the_centre(model):
    """iq_pointnet_coalitions_crt on masked coalitions: every arg-max index is a kept point of that coalition or N (the centre
    that masked points collapse to), and it is consistent with the dense forward on the materialised cloud where the maximum is
    attained by a kept point."""
    d = dev()
    pts, _ = synth.make_cloud(6)
    data = torch.from_numpy(pts).unsqueeze(0).to(d)
    center = torch.mean(data, dim=1)
    rid = hip_ops.region_assign(data[0].contiguous(), hip_ops.fps(data, 8)[0].contiguous())
    keep_list = [0x0f, 0xf0, 0xff, 0x01]
    keep = hip_ops.masks_to_tensor(keep_list, d)
    eng = model.engine()
    logits, crt = eng.coalition_logits(data, center, rid.reshape(1, -1), keep, None, num_regions=8, return_crt=True)
    crt = crt.cpu().numpy()
    rid_np = rid.cpu().numpy()
    for b, k in enumerate(keep_list):
        kept = ((k >> rid_np) & 1).astype(bool)
        ok = (crt[b] == 1024) | kept[np.minimum(crt[b], 1023)]
        assert ok.all()
        if k == 0xff:
            assert (crt[b] < 1024).all()                       # nothing masked: no centre row
    masked = torch.from_numpy(masked_by_keep(pts, rid_np, keep_list, center[0].cpu().numpy())).permute(0, 2, 1).contiguous().to(d)
    dense_logits, _, dense_crt = model(masked)
    assert torch.equal(dense_logits, logits)                    # fused == dense, still bitwise with the arg-max variant
    dense_crt = dense_crt.cpu().numpy()
    for b, k in enumerate(keep_list):
        kept = ((k >> rid_np) & 1).astype(bool)
        at_kept = crt[b] < 1024
        # in the materialised cloud a masked point sits at the centre: where the coalition's arg-max is a kept point the dense
        # forward finds the same point unless a masked copy of the centre ties... compare only channels won by kept points on both sides
        both = at_kept & kept[np.minimum(dense_crt[b], 1023)]
        assert (crt[b][both] == dense_crt[b][both]).mean() > 0.99
