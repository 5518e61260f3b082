"""GPU parity of the standalone geometric ops (include/iq.h: iq_index_points .. iq_density) and of the reference's
`models.*` helpers built on them, against the CPU oracle and the golden vectors from the reference.  Gathers only copy and
subtract, so they are compared bit for bit; kNN is index-valued, so sets may differ only by candidates at a numerical tie."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from probes import assert_rows_nearest_first, set_mismatches
from interpret_quality_amd import _lib, hip_ops, synth

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def oracle():
    from oracle import ref_cpu
    return ref_cpu


def masked(name, oracle):
    """The 18 masked clouds the golden generator of `name` ran on (shapley_masked_batch of cloud 0)."""
    g = load_golden(name)
    data = torch.from_numpy(synth.make_cloud(0)[0]).unsqueeze(0)
    center = torch.mean(data, dim=1).squeeze()
    return oracle.shapley_masked_batch(data, center, g["orders"], g["region_id"])  # (18,1024,3)


def assert_bitwise(got, want):
    got, want = got.detach().cpu().contiguous(), want.detach().cpu().contiguous()
    assert got.shape == want.shape, (got.shape, want.shape)
    assert got.dtype == want.dtype == torch.float32
    assert np.array_equal(got.numpy().view(np.uint32), want.numpy().view(np.uint32))


def long(a):
    return torch.from_numpy(np.asarray(a).astype(np.int64))


# ---- grouping ------------------------------------------------------------------------------------------------------------

def test_grouping_pointnet2_sa1_sa2_sa3(oracle):
    from models import pointnet2 as M
    g = load_golden("pointnet2.npz")
    sel = list(g["sel"])
    xyz = masked("pointnet2.npz", oracle)[sel].contiguous()              # (3,1024,3)
    d = dev()
    fps1 = long(g["fps1"][sel])
    new_xyz = oracle.index_points(xyz, fps1)
    assert_bitwise(M.index_points(xyz.to(d), fps1.to(d)), new_xyz)
    for r, k in ((0.1, 16), (0.2, 32), (0.4, 128)):                     # sa1: relative xyz only
        idx = long(g["sa1_ball_r%g" % r])
        want = oracle.index_points(xyz, idx) - new_xyz.view(3, 512, 1, 3)
        assert_bitwise(hip_ops.group_points(xyz.to(d), None, new_xyz.to(d), idx.to(d)), want)
    new_xyz2 = oracle.index_points(new_xyz, long(g["fps2"][sel]))
    feats = torch.randn(3, 512, 320, generator=torch.Generator().manual_seed(1))
    for r, k in ((0.2, 32), (0.4, 64), (0.8, 128)):                     # sa2: features first (PointNetSetAbstractionMsg :222-230)
        idx = long(g["sa2_ball_r%g" % r])
        want = torch.cat([oracle.index_points(feats, idx), oracle.index_points(new_xyz, idx) - new_xyz2.view(3, 128, 1, 3)], dim=-1)
        got = hip_ops.group_points(new_xyz.to(d), feats.to(d), new_xyz2.to(d), idx.to(d), xyz_first=False)
        assert_bitwise(got, want)
    feats3 = torch.randn(3, 128, 640, generator=torch.Generator().manual_seed(2))
    new3, grouped3 = M.sample_and_group_all(new_xyz2.to(d), feats3.to(d))   # sa3: group all, absolute xyz first
    assert_bitwise(grouped3, torch.cat([new_xyz2.view(3, 1, 128, 3), feats3.view(3, 1, 128, 640)], dim=-1))
    assert new3.shape == (3, 1, 3) and not new3.abs().any()


def test_grouping_pointconv_group_all_and_knn_groups(oracle):
    from models import pointconv as M
    d = dev()
    xyz = masked("pointconv.npz", oracle)[:4].contiguous()
    feats = torch.randn(4, 1024, 64, generator=torch.Generator().manual_seed(3))
    mean = xyz.mean(dim=1, keepdim=True)
    want = torch.cat([xyz.view(4, 1, 1024, 3) - mean.view(4, 1, 1, 3), feats.view(4, 1, 1024, 64)], dim=-1)
    assert_bitwise(hip_ops.group_points(xyz.to(d), feats.to(d), mean.to(d), None), want)     # idx = NULL
    new_xyz, new_points, grouped_xyz = M.sample_and_group_all(xyz.to(d), feats.to(d))
    c = new_xyz.cpu()
    assert_bitwise(new_points, torch.cat([xyz.view(4, 1, 1024, 3) - c.view(4, 1, 1, 3), feats.view(4, 1, 1024, 64)], dim=-1))
    assert_bitwise(grouped_xyz, xyz.view(4, 1, 1024, 3) - c.view(4, 1, 1, 3))
    # sample_and_group: FPS + kNN + grouping, against the oracle's composition on the same indices
    new_xyz, new_points, gxn, idx = M.sample_and_group(512, 32, xyz.to(d), feats.to(d))
    assert idx.dtype == torch.long and idx.shape == (4, 512, 32)
    ic = idx.cpu()
    nx = oracle.index_points(xyz, oracle.farthest_point_sample(xyz, 512))
    assert_bitwise(new_xyz, nx)
    rel = oracle.index_points(xyz, ic) - nx.view(4, 512, 1, 3)
    assert_bitwise(gxn, rel)
    assert_bitwise(new_points, torch.cat([rel, oracle.index_points(feats, ic)], dim=-1))


@pytest.mark.parametrize("n", [100, 1024, 4096])
def test_gathers_random_indices_with_repeats(n, oracle):
    rng = np.random.default_rng(n)
    d = dev()
    pts = torch.from_numpy(rng.standard_normal((2, n, 5)).astype(np.float32))
    xyz = torch.from_numpy(rng.standard_normal((2, n, 3)).astype(np.float32))
    idx = long(rng.integers(0, n, size=(2, 7, 9)))
    idx[:, 0, :] = idx[:, 0, :1]                                      # repeats
    assert_bitwise(hip_ops.index_points(pts.to(d), idx.to(d)), oracle.index_points(pts, idx))
    assert_bitwise(hip_ops.index_points(pts.to(d), idx[:, :, 0].to(d)), oracle.index_points(pts, idx[:, :, 0]))
    ctr = torch.from_numpy(rng.standard_normal((2, 7, 3)).astype(np.float32))
    want = torch.cat([oracle.index_points(xyz, idx) - ctr.view(2, 7, 1, 3), oracle.index_points(pts, idx)], dim=-1)
    assert_bitwise(hip_ops.group_points(xyz.to(d), pts.to(d), ctr.to(d), idx.to(d)), want)
    p8 = torch.from_numpy(rng.standard_normal((2, n, 8)).astype(np.float32))          # C % 4 == 0: the 16-byte path
    assert_bitwise(hip_ops.index_points(p8.to(d), idx.to(d)), oracle.index_points(p8, idx))


# ---- edge features ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", [3, 5, 64, 128])
def test_edge_features_bitwise_both_layouts(c, oracle):
    from models.dgcnn import get_graph_feature
    rng = np.random.default_rng(c)
    d = dev()
    x = torch.from_numpy(rng.standard_normal((2, c, 256)).astype(np.float32))
    idx = long(rng.integers(0, 256, size=(2, 256, 20)))
    want = oracle.get_graph_feature(x, 20, idx)
    assert_bitwise(hip_ops.edgeconv_gather(x.to(d), idx.to(d), channel_first=True), want)
    assert_bitwise(hip_ops.edgeconv_gather(x.transpose(2, 1).contiguous().to(d), idx.to(d), channel_first=False), want)
    assert_bitwise(get_graph_feature(x.to(d), k=20, idx=idx.to(d)), want)


# ---- ordered kNN (DGCNN) ---------------------------------------------------------------------------------------------------

def pairwise(x_cf):
    """models/dgcnn.py:13-15 in float32 on the CPU: -|x_i|^2 - (-2 x_i.x_j) - |x_j|^2 (largest = nearest)."""
    inner = torch.matmul(x_cf.transpose(2, 1), x_cf) * -2
    xx = torch.sum(x_cf ** 2, dim=1, keepdim=True)
    return (-xx - inner - xx.transpose(2, 1)).numpy()


def test_dgcnn_knn_is_ordered_like_the_reference(oracle):
    from models.dgcnn import get_graph_feature, knn
    g = load_golden("dgcnn.npz")
    d = dev()
    x_cf = torch.from_numpy(synth.make_cloud(0)[0]).unsqueeze(0).permute(0, 2, 1).contiguous()   # (1,3,1024)
    got = knn(x_cf.to(d), 20)
    assert got.dtype == torch.long
    assert np.array_equal(got.cpu().numpy(), g["knn_xyz"][:1].astype(np.int64))     # element by element: sorted like topk
    assert_bitwise(get_graph_feature(x_cf.to(d)), oracle.get_graph_feature(x_cf, 20))
    # feature space (C = 64): the oracle's layer-1 output; sets modulo ties, rows nearest first
    with torch.no_grad():
        _, aux = oracle.dgcnn_forward(synth.to_torch(synth.dgcnn_state_dict(0)), x_cf, 20, False, return_aux=True)
    x1 = aux["x1"].contiguous()                                                       # (1,64,1024)
    got64 = knn(x1.to(d), 20).cpu().numpy()
    score = pairwise(x1)
    assert set_mismatches(got64, g["knn_feat64"][:1].astype(np.int64), score, 2e-6) <= 8
    assert_rows_nearest_first(got64, -score, 2e-6)


# ---- PointConv kNN ---------------------------------------------------------------------------------------------------------

def test_knn_point_matches_golden(oracle):
    from models.pointconv import knn_point
    g = load_golden("pointconv.npz")
    d = dev()
    xyz = masked("pointconv.npz", oracle)[list(g["sel"])].contiguous()
    new_xyz = oracle.index_points(xyz, oracle.farthest_point_sample(xyz, 512))
    got = knn_point(32, xyz.to(d), new_xyz.to(d)).cpu().numpy()
    dist = oracle.square_distance(new_xyz, xyz).numpy()
    # the masked clouds hold many copies of the centre: those rows tie exactly, and either copy is right
    set_mismatches(got, g["knn_sa1"].astype(np.int64), -dist, 1e-6)
    assert_rows_nearest_first(got, dist, 1e-6)


@pytest.mark.parametrize("n", [64, 100, 2500])
def test_knn_point_against_oracle(n, oracle):
    from models.pointconv import knn_point
    rng = np.random.default_rng(n)
    d = dev()
    xyz = torch.from_numpy(rng.standard_normal((2, n, 3)).astype(np.float32))
    new_xyz = torch.from_numpy(rng.standard_normal((2, 33, 3)).astype(np.float32))
    dist = oracle.square_distance(new_xyz, xyz).numpy()
    for k in sorted({1, 32, 128, n}):
        if k > min(n, 128):
            continue
        got = knn_point(k, xyz.to(d), new_xyz.to(d)).cpu().numpy()
        assert got.shape == (2, 33, k)
        assert set_mismatches(got, oracle.knn_point(k, xyz, new_xyz).numpy(), -dist, 1e-6) <= 2
        assert_rows_nearest_first(got, dist, 1e-6)
        assert (np.sort(got, axis=2)[:, :, 1:] != np.sort(got, axis=2)[:, :, :-1]).all()


def test_knn_point_limits_are_refused():
    d = dev()
    xyz = torch.zeros((1, 200, 3), device=d)
    with pytest.raises(_lib.IqError):
        hip_ops.knn_point(xyz, xyz[:, :4].contiguous(), 129)
    with pytest.raises(_lib.IqError):
        hip_ops.knn_point(torch.zeros((1, 4097, 3), device=d), xyz[:, :4].contiguous(), 4)


# ---- density -----------------------------------------------------------------------------------------------------------------

def test_density_matches_golden_and_oracle(oracle):
    from models.pointconv import compute_density
    g = load_golden("pointconv.npz")
    d = dev()
    xyz = masked("pointconv.npz", oracle)[list(g["sel"])].contiguous()
    got = compute_density(xyz.to(d), 0.1).cpu().numpy()
    assert np.abs(got / g["density_sa1"] - 1).max() <= 2e-6
    rng = np.random.default_rng(5)
    for n, bw in ((100, 0.1), (2500, 0.2), (1024, 0.4)):
        x = torch.from_numpy((0.5 * rng.standard_normal((2, n, 3))).astype(np.float32))
        want = oracle.compute_density(x, bw).numpy()
        got = compute_density(x.to(d), bw).cpu().numpy()
        assert np.abs(got / want - 1).max() <= 2e-6, (n, bw)


# ---- index validation and stream order ---------------------------------------------------------------------------------

@pytest.mark.parametrize("bad", [-1, 50])
def test_out_of_range_indices_raise_before_launch(bad):
    from models import pointnet2
    d = dev()
    n = 50
    pts = torch.randn((2, n, 5), device=d)
    xyz = torch.randn((2, n, 3), device=d)
    idx = torch.randint(0, n, (2, 4, 6), device=d)
    idx[1, 2, 3] = bad
    with pytest.raises(_lib.IqError):
        hip_ops.index_points(pts, idx)
    with pytest.raises(_lib.IqError):
        pointnet2.index_points(pts, idx)
    with pytest.raises(_lib.IqError):
        hip_ops.group_points(xyz, pts, xyz[:, :4].contiguous(), idx)
    eidx = torch.randint(0, n, (2, n, 6), device=d)
    eidx[0, 7, 1] = bad
    with pytest.raises(_lib.IqError):
        hip_ops.edgeconv_gather(pts.transpose(2, 1).contiguous(), eidx)
    with pytest.raises(_lib.IqError):
        hip_ops.sort_neighbours(pts, pts, eidx.to(torch.int32))


def test_batch_and_shape_mismatches_raise_before_launch():
    """Every operand's batch (and the shapes the kernels index by) must agree with the others: no launch otherwise."""
    from models import pointnet2
    d = dev()
    pts = torch.randn((2, 50, 5), device=d)
    xyz = torch.randn((2, 50, 3), device=d)
    for b in (1, 3):                                                      # idx batch below and above B = 2
        idx = torch.randint(0, 50, (b, 4), device=d)
        gidx = torch.randint(0, 50, (b, 4, 6), device=d)
        with pytest.raises(_lib.IqError):
            hip_ops.index_points(pts, idx)
        with pytest.raises(_lib.IqError):
            pointnet2.index_points(pts, idx)
        with pytest.raises(_lib.IqError):
            hip_ops.group_points(xyz, pts, xyz[:, :4].contiguous(), gidx)
        with pytest.raises(_lib.IqError):
            hip_ops.group_points(xyz, None, None, gidx)
        with pytest.raises(_lib.IqError):
            hip_ops.edgeconv_gather(pts.transpose(2, 1).contiguous(), torch.randint(0, 50, (b, 50, 6), device=d))
        with pytest.raises(_lib.IqError):
            hip_ops.knn_point(xyz, torch.randn((b, 4, 3), device=d), 4)
        with pytest.raises(_lib.IqError):
            hip_ops.sort_neighbours(torch.randn((b, 4, 3), device=d), xyz, torch.randint(0, 50, (2, 4, 6), device=d, dtype=torch.int32))
        with pytest.raises(_lib.IqError):
            hip_ops.sort_neighbours(xyz[:, :4].contiguous(), xyz, torch.randint(0, 50, (b, 4, 6), device=d, dtype=torch.int32))
    sidx = torch.randint(0, 50, (2, 4, 6), device=d, dtype=torch.int32)
    with pytest.raises(_lib.IqError):
        hip_ops.sort_neighbours(pts[:, :4].contiguous(), xyz, sidx)       # q has another C than keys
    with pytest.raises(_lib.IqError):
        hip_ops.sort_neighbours(xyz[:, :4].contiguous(), xyz, sidx[:, :3].contiguous())   # idx has another S than q
    with pytest.raises(_lib.IqError):
        hip_ops.knn_point(xyz, pts[:, :4].contiguous(), 4)               # queries are not 3-D points
    with pytest.raises(_lib.IqError):
        hip_ops.group_points(xyz, pts[:1], xyz[:, :4].contiguous(), torch.randint(0, 50, (2, 4, 6), device=d))
    with pytest.raises(_lib.IqError):
        hip_ops.density(pts, 0.1)


def test_int64_indices_outside_the_int32_range_raise():
    """A torch.long index that the int32 cast would wrap into [0, N) is refused, as the reference's indexing refuses it."""
    d = dev()
    pts = torch.randn((2, 50, 5), device=d)
    for bad in (2 ** 32 + 5, -(2 ** 32) + 5):
        idx = torch.randint(0, 50, (2, 4, 6), device=d)
        idx[1, 1, 1] = bad
        with pytest.raises(_lib.IqError):
            hip_ops.index_points(pts, idx)
        with pytest.raises(_lib.IqError):
            hip_ops.group_points(pts[:, :, :3].contiguous(), None, None, idx)
        eidx = torch.randint(0, 50, (2, 50, 6), device=d)
        eidx[0, 3, 2] = bad
        with pytest.raises(_lib.IqError):
            hip_ops.edgeconv_gather(pts.transpose(2, 1).contiguous(), eidx)


def test_sort_neighbours_ties_go_to_the_lower_index():
    d = dev()
    xyz = torch.randn((1, 64, 3), device=d)
    xyz[0, 40] = xyz[0, 7]                                                # an exact duplicate of point 7
    idx = torch.tensor([[[40, 7, 3, 5]]], dtype=torch.int32, device=d)
    got = hip_ops.sort_neighbours(xyz[:, 7:8].contiguous(), xyz, idx).cpu().numpy()[0, 0]
    assert list(got[:2]) == [7, 40]


def test_ops_on_a_non_default_stream(oracle):
    d = dev()
    rng = np.random.default_rng(11)
    xyz_c = torch.from_numpy(rng.standard_normal((2, 256, 3)).astype(np.float32))
    pts_c = torch.from_numpy(rng.standard_normal((2, 256, 6)).astype(np.float32))
    idx_c = long(rng.integers(0, 256, size=(2, 16, 20)))
    eidx_c = long(rng.integers(0, 256, size=(2, 256, 20)))
    xyz, pts, idx, eidx = xyz_c.to(d), pts_c.to(d), idx_c.to(d), eidx_c.to(d)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        r_index = hip_ops.index_points(pts, idx)
        r_group = hip_ops.group_points(xyz, pts, xyz[:, :16].contiguous(), idx)
        r_edge = hip_ops.edgeconv_gather(pts.transpose(2, 1).contiguous(), eidx)
        r_knn = hip_ops.knn_point(xyz, xyz[:, :16].contiguous(), 20)
        r_sort = hip_ops.sort_neighbours(xyz[:, :16].contiguous(), xyz, r_knn.flip(-1).contiguous())
        r_dens = hip_ops.density(xyz, 0.3)
    s.synchronize()
    assert_bitwise(r_index, oracle.index_points(pts_c, idx_c))
    assert_bitwise(r_group, torch.cat([oracle.index_points(xyz_c, idx_c) - xyz_c[:, :16].reshape(2, 16, 1, 3),
                                       oracle.index_points(pts_c, idx_c)], dim=-1))
    assert_bitwise(r_edge, oracle.get_graph_feature(pts_c.transpose(2, 1).contiguous(), 20, eidx_c))
    assert torch.equal(r_sort.cpu(), hip_ops.sort_neighbours(xyz[:, :16].contiguous(), xyz, r_knn.clone()).cpu())
    assert torch.equal(r_sort.sort(-1)[0].cpu(), r_knn.sort(-1)[0].cpu())
    dist = oracle.square_distance(xyz_c[:, :16], xyz_c).numpy()
    set_mismatches(r_knn.cpu().numpy(), oracle.knn_point(20, xyz_c, xyz_c[:, :16]).numpy(), -dist, 1e-6)
    assert np.abs(r_dens.cpu().numpy() / oracle.compute_density(xyz_c, 0.3).numpy() - 1).max() <= 2e-6
