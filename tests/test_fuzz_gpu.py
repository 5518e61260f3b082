"""A seeded slice of the randomised probes (tests/fuzz_sizes.py, tests/fuzz_hotpath.py) and of the standalone geometric ops at
the sizes where their kernels change shape: coalition paths of the five families against the dense HIP forward and the CPU
oracle, the PointNet hot path against the oracle's loop, and iq_knn_point / iq_density / iq_sort_neighbours / the gathers /
iq_fps / iq_ball_query against plain float64 or indexing references, and those ops again on clouds at the ends of the pose sweeps'
grids.  The case lists are built at collection time from fixed seeds plus explicit boundary cases; every id reruns alone with
-k <id>."""
import numpy as np
import pytest
import torch

import probes
from conftest import assert_close_elementwise
from interpret_quality_amd import hip_ops

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


# ---- (a) coalition paths of the five families ---------------------------------------------------------------------------

C = probes.CoalitionCase
COALITION_BOUNDARY = [
    # each family's minimum and minimum + 1
    C("pointnet", 1, 1, 1, 2, 1), C("pointnet", 2, 2, 2, 17, 2),
    C("pointnet2", 128, 8, 1, 9, 3), C("pointnet2", 129, 8, 2, 16, 4),
    C("pointconv", 64, 8, 1, 9, 5), C("pointconv", 65, 8, 3, 17, 6),
    C("dgcnn", 21, 8, 1, 9, 7), C("dgcnn", 22, 2, 2, 5, 8),
    C("gcnn", 21, 8, 1, 9, 9), C("gcnn", 22, 32, 2, 12, 10),
    # the DGCNN range of the round-5 bug (21 - 38 points)
    C("dgcnn", 27, 8, 3, 30, 11), C("dgcnn", 33, 64, 1, 12, 12), C("dgcnn", 38, 8, 2, 20, 13),
    # PointConv's sa1 keeps 512 points: below it sampling repeats index 0
    C("pointconv", 511, 8, 1, 8, 14), C("pointconv", 512, 8, 1, 8, 15),
    # both sides of 32, 1024 and 2048
    C("pointnet", 31, 8, 1, 8, 16), C("pointnet", 33, 8, 2, 16, 17), C("gcnn", 32, 8, 1, 8, 18), C("dgcnn", 33, 8, 1, 6, 19),
    C("pointnet", 1023, 32, 1, 8, 20), C("pointnet", 1025, 32, 1, 8, 21), C("pointnet2", 1024, 8, 1, 4, 22),
    C("pointconv", 1024, 8, 1, 4, 23), C("pointconv", 1025, 8, 1, 4, 24), C("dgcnn", 1025, 8, 1, 3, 25),
    C("pointnet", 2047, 8, 1, 4, 26), C("pointnet", 2049, 8, 1, 4, 27), C("pointnet2", 2049, 8, 1, 3, 28),
    C("gcnn", 2048, 8, 1, 3, 29),
    # PointNet's largest cloud
    C("pointnet", 4096, 8, 1, 2, 30),
    # one region and 64; 9 source clouds (no pair tables); 8 and more coalitions per source cloud (source-list groups)
    C("pointnet", 300, 1, 3, 24, 31), C("pointnet2", 200, 1, 2, 4, 32), C("pointnet", 500, 64, 2, 20, 33),
    C("pointconv", 100, 64, 1, 9, 34), C("gcnn", 60, 64, 9, 72, 35), C("pointnet", 129, 8, 9, 81, 36),
    C("pointnet2", 150, 8, 9, 72, 37), C("dgcnn", 50, 2, 3, 24, 38),
]
COALITION_RANDOM = [probes.random_coalition_case(rng, f) for rng in [np.random.default_rng(2024)] for f in probes.FAMILIES * 2]
COALITION_CASES = COALITION_BOUNDARY + COALITION_RANDOM
ORACLE_CAP = 8192                 # the CPU oracle runs on cases of at most this many points (coalitions x N) in all


@pytest.mark.parametrize("case", COALITION_CASES, ids=[c.id for c in COALITION_CASES])
def test_coalition_path_random_shapes(case):
    got, dense, want, _ = probes.run_coalition_case(case, dev(), oracle_cap=ORACLE_CAP)
    assert got.shape[0] == case.b and got.shape == dense.shape
    problems = probes.coalition_problems(case.family, got, dense, want)
    assert not problems, problems
    if want is not None and case.family != "dgcnn":
        assert_close_elementwise(got, want)


# ---- (b) the hot path (PointNet) ------------------------------------------------------------------------------------------

H = probes.HotpathCase
HOT_BOUNDARY = [
    H(8, 1, 1, 1, "modified", 1), H(8, 64, 1, 1, "normal", 2), H(8, 3, 4, 2, "modified", 3),
    H(4096, 2, 3, 3, "modified", 4), H(4096, 17, 2, 1, "normal", 5), H(4096, 1, 2, 2, "normal", 6),
    H(513, 64, 2, 2, "modified", 7), H(1000, 3, 6, 2, "normal", 8), H(100, 17, 3, 3, "modified", 9),
    H(33, 2, 3, 1, "normal", 10),
]
HOT_ORACLE_POINTS = 200_000       # s * (R + 1) * N: what the oracle's loop pushes through the CPU forward


def _hot_random(seed, count):
    rng, out = np.random.default_rng(seed), []
    while len(out) < count:
        c = probes.random_hotpath_case(rng)
        if c.s * (c.r + 1) * c.n <= HOT_ORACLE_POINTS:
            out.append(c)
    return out


HOT_CASES = HOT_BOUNDARY + _hot_random(2024, 6)


@pytest.mark.parametrize("case", HOT_CASES, ids=[c.id for c in HOT_CASES])
def test_hot_path_random_shapes(case):
    res = probes.run_hotpath_case(case, dev())
    assert np.array_equal(res["fps"], res["want_fps"])                      # FPS bit for bit
    problems = probes.hotpath_problems(res)
    assert not problems, problems


# ---- (c) standalone geometric ops against plain references ---------------------------------------------------------------

def _cloud(rng, b, n, scale=1.0):
    return (scale * rng.standard_normal((b, n, 3))).astype(np.float32)


KNN_CASES = [(b, n, s) for b, n, s in [
    (1, 1, 1), (3, 2, 7), (1, 63, 33), (3, 64, 1), (1, 65, 128), (3, 1023, 50), (1, 1024, 600), (3, 1025, 17),
    (1, 4095, 1), (3, 4096, 300), (1, 300, 257), (3, 2600, 90)]]


@pytest.mark.parametrize("b,n,s", KNN_CASES, ids=["knn-B%d-N%d-S%d" % c for c in KNN_CASES])
def test_knn_point_random_shapes(b, n, s):
    rng = np.random.default_rng(1000 * n + s)
    xyz = _cloud(rng, b, n)
    new_xyz = _cloud(rng, b, s)
    new_xyz[:, ::3] = xyz[:, rng.integers(0, n, size=new_xyz[:, ::3].shape[1])]     # some queries ON a cloud point
    kmax = min(n, 128)
    for k in sorted({1, kmax, int(rng.integers(1, kmax + 1))}):
        got = hip_ops.knn_point(torch.from_numpy(xyz).to(dev()), torch.from_numpy(new_xyz).to(dev()), k).cpu().numpy()
        nbad = probes.check_knn(got, xyz, new_xyz, k)
        assert nbad <= max(2, b * s // 100), (k, nbad)


def test_knn_point_duplicate_points_lower_index_first():
    rng = np.random.default_rng(7)
    xyz = _cloud(rng, 2, 700)
    for b in range(2):                          # groups of up to 6 exact copies scattered over the index range
        for _ in range(60):
            src = int(rng.integers(0, 700))
            xyz[b, rng.integers(0, 700, size=int(rng.integers(1, 6)))] = xyz[b, src]
    new_xyz = np.concatenate([xyz[:, :40], _cloud(rng, 2, 40, 0.2)], axis=1)
    for k in (1, 5, 64, 128):
        got = hip_ops.knn_point(torch.from_numpy(xyz).to(dev()), torch.from_numpy(new_xyz).to(dev()), k).cpu().numpy()
        probes.check_knn(got, xyz, new_xyz, k)
        probes.assert_duplicates_lower_index_first(got, xyz)


DENSITY_CASES = [(1, 1, 0.05), (2, 2, 0.1), (5, 255, 0.4), (2, 256, 2.0), (5, 257, 0.05), (1, 1023, 0.1),
                 (2, 1024, 0.4), (5, 1025, 0.1), (2, 2049, 0.05), (1, 4096, 0.4), (1, 4096, 2.0)]


def _ball(rng, b, n, radius):
    """Points uniform in a ball of `radius` (|x|^2 small keeps the float32 expanded-form distance well inside 1e-4)."""
    d = rng.standard_normal((b, n, 3))
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    return (radius * d * rng.random((b, n, 1)) ** (1 / 3)).astype(np.float32)


@pytest.mark.parametrize("b,n,bw", DENSITY_CASES, ids=["density-B%d-N%d-h%g" % c for c in DENSITY_CASES])
def test_density_random_shapes(b, n, bw):
    from oracle import ref_cpu as O
    rng = np.random.default_rng(n + b)
    x = _ball(rng, b, n, 0.5)
    got = hip_ops.density(torch.from_numpy(x).to(dev()), bw).cpu().numpy()
    problems = probes.density_problems(got, O.compute_density(torch.from_numpy(x), bw).numpy(), probes.density64(x, bw))
    assert not problems, problems


SORT_CASES = [(b, s, c, k) for b, s, c, k in [
    (1, 1, 1, 1), (1, 2, 3, 2), (3, 1, 5, 20), (1, 7, 64, 63), (2, 5, 128, 64), (3, 3, 200, 65), (1, 11, 3, 127),
    (5, 3, 64, 128), (2, 9, 3, 64)]]


@pytest.mark.parametrize("b,s,c,k", SORT_CASES, ids=["sort-B%d-S%d-C%d-k%d" % c for c in SORT_CASES])
def test_sort_neighbours_random_shapes(b, s, c, k):
    assert (b * s) % 4 != 0                                                   # a partly filled last workgroup
    rng = np.random.default_rng(b * 1000 + s * 100 + c + k)
    n = int(rng.integers(max(2, k // 2), 4097))
    keys = rng.standard_normal((b, n, c)).astype(np.float32)
    for bb in range(b):                                                       # coinciding points
        keys[bb, rng.integers(0, n, size=n // 8)] = keys[bb, int(rng.integers(0, n))]
    q = rng.standard_normal((b, s, c)).astype(np.float32)
    q[:, 0] = keys[:, 0]                                                      # a query on a key
    idx = rng.integers(0, n, size=(b, s, k)).astype(np.int32)
    idx[:, ::2, : k // 2] = idx[:, ::2, :1]                                   # repeated entries
    got = hip_ops.sort_neighbours(torch.from_numpy(q).to(dev()), torch.from_numpy(keys).to(dev()),
                                  torch.from_numpy(idx.copy()).to(dev())).cpu().numpy()
    probes.check_sorted_rows(got, idx, q, keys)


GATHER_CASES = [(c, b, n, s, k) for c, b, n, s, k in [
    (1, 1, 5, 3, 3), (2, 2, 17, 5, 7), (3, 3, 100, 7, 5), (4, 1, 33, 9, 1), (5, 2, 64, 3, 11), (7, 1, 257, 13, 3),
    (8, 3, 50, 5, 3), (64, 1, 130, 3, 5), (131, 2, 40, 1, 3)]]


def _unaligned(a, d):
    """A contiguous device copy of `a` that starts 4 bytes into a larger buffer (not 16-byte aligned)."""
    buf = torch.zeros(a.size + 4, dtype=torch.float32, device=d)
    v = buf[1:1 + a.size].view(a.shape)
    v.copy_(torch.from_numpy(a))
    assert v.is_contiguous() and v.data_ptr() % 16 != 0
    return v


def _torch_rows(t, idx):
    return t[torch.arange(t.shape[0]).view(-1, *([1] * (idx.dim() - 1))), idx]


@pytest.mark.parametrize("c,b,n,s,k", GATHER_CASES, ids=["gather-C%d-B%d-N%d-S%d-K%d" % g for g in GATHER_CASES])
def test_gathers_random_shapes_and_unaligned_points(c, b, n, s, k):
    from oracle import ref_cpu as O
    d = dev()
    rng = np.random.default_rng(c * 100 + n)
    pts = rng.standard_normal((b, n, c)).astype(np.float32)
    xyz = rng.standard_normal((b, n, 3)).astype(np.float32)
    ctr = rng.standard_normal((b, s, 3)).astype(np.float32)
    idx2 = torch.from_numpy(rng.integers(0, n, size=(b, s)))
    idx3 = torch.from_numpy(rng.integers(0, n, size=(b, s, k)))
    P, X, T = torch.from_numpy(pts), torch.from_numpy(xyz), torch.from_numpy(ctr)
    for points in (P.to(d), _unaligned(pts, d)):
        for idx in (idx2, idx3):
            assert probes.bitwise_equal(hip_ops.index_points(points, idx.to(d)).cpu(), _torch_rows(P, idx))
        rel = _torch_rows(X, idx3) - T.view(b, s, 1, 3)
        for xyz_first in (True, False):
            want = torch.cat([rel, _torch_rows(P, idx3)] if xyz_first else [_torch_rows(P, idx3), rel], dim=-1)
            got = hip_ops.group_points(X.to(d), points, T.to(d), idx3.to(d), xyz_first=xyz_first).cpu()
            assert probes.bitwise_equal(got, want), xyz_first
    assert probes.bitwise_equal(hip_ops.group_points(X.to(d), None, T.to(d), idx3.to(d)).cpu(), rel)        # D = 0
    assert probes.bitwise_equal(hip_ops.group_points(X.to(d), None, None, idx3.to(d)).cpu(), _torch_rows(X, idx3))
    eidx = torch.from_numpy(rng.integers(0, n, size=(b, n, k)))
    want = O.get_graph_feature(P.transpose(2, 1).contiguous(), k, eidx)
    assert probes.bitwise_equal(hip_ops.edgeconv_gather(P.to(d), eidx.to(d), channel_first=False).cpu(), want)
    assert probes.bitwise_equal(hip_ops.edgeconv_gather(P.transpose(2, 1).contiguous().to(d), eidx.to(d), channel_first=True).cpu(), want)
    assert probes.bitwise_equal(hip_ops.edgeconv_gather(_unaligned(pts, d), eidx.to(d), channel_first=False).cpu(), want)


FPS_CASES = [(1, 1, 1, False), (1, 2, 2, False), (64, 2, 5, False), (63, 127, 127, True), (64, 128, 128, False),
             (65, 129, 64, True), (63, 511, 100, False), (64, 512, 512, True), (65, 513, 64, False), (64, 1023, 100, True),
             (65, 1024, 1024, False), (64, 1025, 64, True), (1, 3072, 3072, False), (2, 3073, 3073, True)]


@pytest.mark.parametrize("b,n,s,collapse", FPS_CASES, ids=["fps-B%d-N%d-S%d%s" % (b, n, s, "-dup" if c else "")
                                                           for b, n, s, c in FPS_CASES])
def test_fps_on_both_sides_of_the_kernel_thresholds(b, n, s, collapse):
    """iq_fps: one wave per cloud for B >= 64 and N <= 128 / 512 / 1024, the workgroup kernel otherwise (more LDS above
    N = 3072); `collapse`: most points of every other cloud coincide, so S exceeds the distinct points."""
    from oracle import ref_cpu as O
    rng = np.random.default_rng(b * 10000 + n)
    x = _cloud(rng, b, n)
    if collapse:
        for i in range(0, b, 2):
            x[i, rng.random(n) < 0.9] = x[i, int(rng.integers(0, n))]
    got = hip_ops.fps(torch.from_numpy(x).to(dev()), s).cpu().numpy()
    assert np.array_equal(got, O.farthest_point_sample(torch.from_numpy(x), s).numpy())


BALL_CASES = [(1, 1, 5, 1), (2, 127, 30, 16), (1, 128, 64, 64), (2, 1024, 100, 128), (1, 1025, 77, 16), (1, 4096, 60, 128),
              (2, 4096, 20, 64)]


@pytest.mark.parametrize("b,n,s,nsample", BALL_CASES, ids=["ball-B%d-N%d-S%d-K%d" % c for c in BALL_CASES])
def test_ball_query_random_shapes(b, n, s, nsample):
    from oracle import ref_cpu as O
    rng = np.random.default_rng(n * 7 + nsample)
    xyz = _ball(rng, b, n, 1.0)
    # centroids on cloud points (FPS picks them so) and just off them: every ball holds a point.  An empty ball is outside
    # the reference's domain - its query_ball_point pads the row with index N, which the next gather cannot index.
    new_xyz = xyz[:, rng.integers(0, n, size=s)].copy()
    new_xyz[:, 1::2] += (0.005 * rng.standard_normal((b, s // 2, 3))).astype(np.float32)
    for radius in (float(rng.uniform(0.05, 0.2)), float(rng.uniform(0.2, 1.0))):
        got = hip_ops.ball_query(torch.from_numpy(xyz).to(dev()), torch.from_numpy(new_xyz).to(dev()), radius, nsample).cpu().numpy()
        X, Q = torch.from_numpy(xyz), torch.from_numpy(new_xyz)
        want = O.query_ball_point(radius, nsample, X, Q).numpy()
        assert want.max() < n                                                 # no empty ball
        assert got.shape == want.shape
        assert probes.ball_mismatch(got, want, X, Q, radius, O) <= max(1, b * s // 100)


# ---- (d) the geometric ops at the ends of the pose sweeps' grids -------------------------------------------------------------

POSED_GEOM = [(n, pose) for n in (100, 513) for pose in ("s0.5", "s2.0", "t+")]


@pytest.mark.parametrize("n,pose", POSED_GEOM, ids=["geom-N%d-%s" % c for c in POSED_GEOM])
def test_geometric_ops_under_sweep_poses(n, pose):
    """One synthetic cloud scaled by 0.5 and 2.0 and translated by 0.5 (f64_cases.POSES): the ops whose float32 expanded-form
    distances carry a larger |x|^2 there - and whose fixed radii and bandwidths meet another point density - under the checkers and
    tolerances of the cases above."""
    import f64_cases as F
    from interpret_quality_amd import synth
    from oracle import ref_cpu as O
    x = F.apply_pose(synth.make_cloud(60 + n, n)[0][None], pose)
    X, xd = torch.from_numpy(x), torch.from_numpy(x).to(dev())
    for bw in (0.1, 0.4):
        got = hip_ops.density(xd, bw).cpu().numpy()
        want32, want64 = O.compute_density(X, bw).numpy(), probes.density64(x, bw)
        e = lambda w: (np.abs(got - w) / np.maximum(np.abs(w), probes.DENSITY_FLOOR)).max()
        print("N=%d %s density h=%g: vs oracle %.3g, vs float64 %.3g (the oracle vs float64 %.3g)" % (
            n, pose, bw, e(want32), e(want64), (np.abs(want32 - want64) / np.abs(want64)).max()))
        problems = probes.density_problems(got, want32, want64)
        assert not problems, (bw, problems)
    s = min(n, 128)
    fps = hip_ops.fps(xd, s)
    want_fps = O.farthest_point_sample(X, s)
    assert np.array_equal(fps.cpu().numpy(), want_fps.numpy())
    new_xyz = x[:, want_fps[0].numpy()]
    Q, qd = torch.from_numpy(new_xyz), torch.from_numpy(new_xyz).to(dev())
    for k in (1, 20, min(n, 128)):
        nbad = probes.check_knn(hip_ops.knn_point(xd, qd, k).cpu().numpy(), x, new_xyz, k)
        assert nbad <= max(2, s // 100), (k, nbad)
    for radius, nsample in ((0.1, 16), (0.2, 32), (0.4, min(n, 128))):      # sa1 of PointNet++ (the reference needs nsample <= N)
        got = hip_ops.ball_query(xd, qd, radius, nsample).cpu().numpy()
        want = O.query_ball_point(radius, nsample, X, Q).numpy()
        assert want.max() < n and got.shape == want.shape
        assert probes.ball_mismatch(got, want, X, Q, radius, O) <= max(1, s // 100), radius
    for r in (8, 32):
        rid = hip_ops.region_assign(xd[0].contiguous(), fps[0, :r].contiguous()).cpu().numpy()
        want_rid = np.asarray(O.cal_region_id(X, want_fps[0, :r]))
        assert rid.shape == (n,) and (rid != want_rid).mean() <= probes.REGION_NEAR_TIE_FRACTION, r
