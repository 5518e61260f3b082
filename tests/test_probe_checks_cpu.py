"""The checkers of tests/probes.py reject subtly wrong answers (no GPU): each gets a right answer built on the host, then one
with a single plausible kernel bug in it.  Also pins the boundary sizes the case lists of tests/test_fuzz_gpu.py must keep."""
import numpy as np
import pytest
import torch

import probes
from conftest import assert_close_elementwise
from oracle import ref_cpu as O


def _rng(seed=0):
    return np.random.default_rng(seed)


# ---- kNN -------------------------------------------------------------------------------------------------------------------

def _knn_setup(k=8):
    rng = _rng(1)
    xyz = rng.standard_normal((2, 200, 3)).astype(np.float32)
    new_xyz = rng.standard_normal((2, 30, 3)).astype(np.float32)
    order = np.argsort(probes.sqdist64(new_xyz, xyz), axis=2, kind="stable")
    return xyz, new_xyz, order[:, :, :k].copy(), order[:, :, k].copy(), k


def test_knn_checker_accepts_the_float64_top_k():
    xyz, new_xyz, right, _, k = _knn_setup()
    assert probes.check_knn(right, xyz, new_xyz, k) == 0


def test_knn_checker_rejects_two_swapped_neighbours():
    xyz, new_xyz, right, _, k = _knn_setup()
    wrong = right.copy()
    wrong[1, 4, [0, k - 1]] = wrong[1, 4, [k - 1, 0]]
    with pytest.raises(AssertionError):
        probes.check_knn(wrong, xyz, new_xyz, k)


def test_knn_checker_rejects_the_k_plus_first_neighbour():
    xyz, new_xyz, right, next_one, k = _knn_setup()
    wrong = right.copy()
    wrong[0, 7, k - 1] = next_one[0, 7]                   # still nearest first, but the wrong set
    with pytest.raises(AssertionError):
        probes.check_knn(wrong, xyz, new_xyz, k)


def test_knn_checker_rejects_a_repeat_and_an_out_of_range_index():
    xyz, new_xyz, right, _, k = _knn_setup()
    wrong = right.copy()
    wrong[0, 2, 1] = wrong[0, 2, 0]
    with pytest.raises(AssertionError):
        probes.check_knn(wrong, xyz, new_xyz, k)
    wrong = right.copy()
    wrong[1, 0, k - 1] = 200
    with pytest.raises(AssertionError):
        probes.check_knn(wrong, xyz, new_xyz, k)


def test_duplicate_order_checker():
    xyz = _rng(2).standard_normal((1, 10, 3)).astype(np.float32)
    xyz[0, 6] = xyz[0, 2]
    probes.assert_duplicates_lower_index_first(np.array([[[2, 6, 0]]]), xyz)
    with pytest.raises(AssertionError):
        probes.assert_duplicates_lower_index_first(np.array([[[6, 2, 0]]]), xyz)        # higher copy first
    with pytest.raises(AssertionError):
        probes.assert_duplicates_lower_index_first(np.array([[[6, 0, 1]]]), xyz)        # lower copy left out


# ---- sorted neighbour rows -----------------------------------------------------------------------------------------------

def test_sorted_rows_checker():
    rng = _rng(3)
    keys = rng.standard_normal((1, 50, 64)).astype(np.float32)
    keys[0, 30] = keys[0, 4]
    q = rng.standard_normal((1, 2, 64)).astype(np.float32)
    inp = rng.integers(0, 50, size=(1, 2, 12)).astype(np.int32)
    inp[0, 0, :3] = [30, 4, 30]
    d = probes.sqdist64(q, keys)
    right = np.stack([np.stack([row[np.lexsort((row, d[0, s, row]))] for s, row in enumerate(inp[0])])])
    probes.check_sorted_rows(right, inp, q, keys)
    wrong = right.copy()
    wrong[0, 1, [0, -1]] = wrong[0, 1, [-1, 0]]
    with pytest.raises(AssertionError):
        probes.check_sorted_rows(wrong, inp, q, keys)                       # not nearest first
    wrong = right.copy()
    wrong[0, 1, 0] = (wrong[0, 1, 0] + 1) % 50
    with pytest.raises(AssertionError):
        probes.check_sorted_rows(wrong, inp, q, keys)                       # not a permutation of the input row
    wrong = right.copy()
    pos = [j for j, v in enumerate(wrong[0, 0]) if v in (4, 30)]
    wrong[0, 0, pos] = wrong[0, 0, pos[::-1]]
    with pytest.raises(AssertionError):
        probes.check_sorted_rows(wrong, inp, q, keys)                       # coinciding points out of index order


# ---- density ---------------------------------------------------------------------------------------------------------------

def _density_setup(n=1100, bw=0.1):
    rng = _rng(4)
    d = rng.standard_normal((2, n, 3))
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    x = (0.5 * d * rng.random((2, n, 1)) ** (1 / 3)).astype(np.float32)
    return x, bw, O.compute_density(torch.from_numpy(x), bw).numpy(), probes.density64(x, bw)


def test_density_checker_accepts_the_oracle():
    x, bw, want32, want64 = _density_setup()
    assert probes.density_problems(want32, want32, want64) == []
    assert probes.density64(x[:, :300], bw).shape == (2, 300)


def test_density_checker_rejects_a_dropped_tile_and_a_wrong_denominator():
    x, bw, want32, want64 = _density_setup()
    n = x.shape[1]
    xd = x.astype(np.float64)
    d = ((xd[:, :, None] - xd[:, None, :1024]) ** 2).sum(-1)                    # the first 1024-point tile only
    tile = (np.exp(-d / (2 * bw * bw)) / (2.5 * bw)).sum(-1) / n
    assert probes.density_problems((want64 - tile).astype(np.float32), want32, want64)        # the first tile left out
    assert probes.density_problems((want64 * n / (n + 1)).astype(np.float32), want32, want64)   # divided by N + 1
    x1 = x[:, :1025]
    w32, w64 = O.compute_density(torch.from_numpy(x1), bw).numpy(), probes.density64(x1, bw)
    assert probes.density_problems((w64 * 1025 / 1026).astype(np.float32), w32, w64)


# ---- gathers and FPS ------------------------------------------------------------------------------------------------------

def test_gather_checker_rejects_a_shifted_index_and_a_zeroed_tail_quad():
    rng = _rng(5)
    pts = torch.from_numpy(rng.standard_normal((2, 40, 5)).astype(np.float32))
    idx = torch.from_numpy(rng.integers(0, 39, size=(2, 7, 3)))
    right = pts[torch.arange(2).view(2, 1, 1), idx]
    assert probes.bitwise_equal(right, right.clone())
    shifted = idx.clone()
    shifted[1, 3, 2] += 1
    assert not probes.bitwise_equal(pts[torch.arange(2).view(2, 1, 1), shifted], right)
    tail = right.clone().reshape(-1)
    total = tail.numel()                                                         # 210 = 4 * 52 + 2: a partial last quad
    assert total % 4 != 0
    tail[total - total % 4:] = 0
    assert not probes.bitwise_equal(tail.view(right.shape), right)


def test_fps_comparison_rejects_a_wrong_start():
    x = torch.from_numpy(_rng(6).standard_normal((1, 64, 3)).astype(np.float32))
    want = O.farthest_point_sample(x, 8).numpy()
    x_rolled = torch.roll(x, -1, dims=1)                                          # the sampler started from point 1
    wrong = (O.farthest_point_sample(x_rolled, 8).numpy() + 1) % 64
    assert wrong[0, 0] == 1 and not np.array_equal(wrong, want)


# ---- coalition logits ------------------------------------------------------------------------------------------------------

def test_coalition_checker_rejects_swapped_rows_and_a_perturbed_row():
    rng = _rng(7)
    want = rng.standard_normal((12, 10)).astype(np.float32) * 5
    assert probes.coalition_problems("pointconv", want.copy(), want, want) == []
    swapped = want.copy()
    swapped[[3, 8]] = swapped[[8, 3]]
    assert probes.coalition_problems("pointconv", swapped, want, want)
    assert probes.coalition_problems("pointconv", want.copy(), swapped, None)     # the dense forward alone catches it too
    rng_ = np.abs(want).max()
    bumped = want.copy()
    bumped[5] += 2e-4 * rng_
    assert probes.coalition_problems("pointnet", bumped, want, None)
    assert probes.coalition_problems("pointnet", want.copy(), want, bumped)
    with pytest.raises(AssertionError):
        assert_close_elementwise(bumped, want)
    nan = want.copy()
    nan[0, 0] = np.nan
    assert probes.coalition_problems("gcnn", nan, want, want)


def test_coalition_checker_holds_dgcnn_to_the_qualified_oracle_bar():
    want = _rng(8).standard_normal((6, 10)).astype(np.float32)
    off = want.copy()
    off[2] += 5e-3 * np.abs(want).max()
    assert probes.coalition_problems("dgcnn", off, off, want) == []               # within 1e-2 of the float32 oracle
    assert probes.coalition_problems("dgcnn", off, want, want)                    # but 1e-4 of the dense HIP forward
    off[2] += 1e-2 * np.abs(want).max()
    assert probes.coalition_problems("dgcnn", off, off, want)


def test_coalition_inputs_hold_the_full_and_the_empty_coalition():
    case = probes.CoalitionCase("pointnet2", 130, 64, 3, 20, 99)
    clouds, rid, keep, cloud_of = probes.coalition_inputs(case)
    assert clouds.shape == (3, 130, 3) and rid.shape == (3, 130) and rid.max() < 64
    assert keep[0] == (1 << 64) - 1 and keep[-1] == 0 and len(keep) == 20
    assert cloud_of.shape == (20,) and cloud_of.max() < 3
    assert case.id == "pointnet2-N130-R64-nc3-b20-s99"


def test_hotpath_errors_flag_a_wrong_fps():
    res = dict(fps=np.array([[0, 5, 9]]), want_fps=np.array([[0, 5, 9]]), region_id=np.zeros(50), want_rid=np.zeros(50),
               logits=np.ones((4, 10)), want_logits=np.ones((4, 10)), phi=np.ones(3), want_phi=np.ones(3),
               int_logits=None, want_int_logits=None, int_v=None, want_int_v=None)
    assert probes.hotpath_problems(res) == []
    assert probes.hotpath_problems(dict(res, fps=np.array([[1, 5, 9]])))
    assert probes.hotpath_problems(dict(res, region_id=np.arange(50) % 2))
    assert probes.hotpath_problems(dict(res, logits=np.ones((4, 10)) + 2e-4))


# ---- the explicit boundary lists of tests/test_fuzz_gpu.py -----------------------------------------------------------------

def test_boundary_lists_hold_the_named_sizes():
    import test_fuzz_gpu as m                                        # builds its case lists at import, without a GPU
    sizes = {(c.family, c.n) for c in m.COALITION_BOUNDARY}
    for fam, lo in (("pointnet", 1), ("pointnet2", 128), ("pointconv", 64), ("dgcnn", 21), ("gcnn", 21)):
        assert (fam, lo) in sizes and (fam, lo + 1) in sizes, fam
    assert {("pointconv", 511), ("pointconv", 512), ("pointnet", 4096)} <= sizes
    ns = {c.n for c in m.COALITION_BOUNDARY}
    for edge in (32, 1024, 2048):
        assert any(n < edge for n in ns if n >= edge - 1) and any(n > edge for n in ns if n <= edge + 1), edge
    dg = sorted(c.n for c in m.COALITION_BOUNDARY if c.family == "dgcnn" and c.n <= 38)
    assert dg[0] == 21 and dg[-1] == 38 and len(dg) >= 5
    assert {1, 64} <= {c.r for c in m.COALITION_BOUNDARY}
    assert any(c.nc == 9 for c in m.COALITION_BOUNDARY)
    assert any(c.b >= 8 * c.nc for c in m.COALITION_BOUNDARY if c.nc > 1)
    assert {1, 2, 3, 17, 64} <= {c.r for c in m.HOT_CASES} and {8, 4096} <= {c.n for c in m.HOT_CASES}
    assert {"modified", "normal"} <= {c.sm for c in m.HOT_CASES}
    assert len({c.id for c in m.COALITION_CASES}) == len(m.COALITION_CASES)
    assert len({c.id for c in m.HOT_CASES}) == len(m.HOT_CASES)

    knn_n = {n for _, n, _ in m.KNN_CASES}
    assert {1, 2, 63, 64, 65, 1023, 1024, 1025, 4095, 4096} <= knn_n and {1, 3} == {b for b, _, _ in m.KNN_CASES}
    assert 1 in {s for _, _, s in m.KNN_CASES} and max(s for _, _, s in m.KNN_CASES) <= 600
    assert {1, 2, 255, 256, 257, 1023, 1024, 1025, 2049, 4096} <= {n for _, n, _ in m.DENSITY_CASES}
    assert {1, 2, 5} <= {b for b, _, _ in m.DENSITY_CASES} and {0.05, 0.1, 0.4, 2.0} <= {h for _, _, h in m.DENSITY_CASES}
    assert {(b * s) % 4 for b, s, _, _ in m.SORT_CASES} == {1, 2, 3}
    assert {1, 3, 5, 64, 128, 200} <= {c for _, _, c, _ in m.SORT_CASES}
    assert {1, 2, 20, 63, 64, 65, 127, 128} <= {k for _, _, _, k in m.SORT_CASES}
    assert {1, 2, 3, 4, 5, 7, 8, 64, 131} <= {c for c, *_ in m.GATHER_CASES}
    totals = set()
    for c, b, n, s, k in m.GATHER_CASES:
        totals |= {b * s * c % 4, b * s * k * c % 4, b * s * k * (3 + c) % 4, b * s * k * 3 % 4, 2 * b * c * n * k % 4}
    assert {1, 2, 3} <= totals
    assert {1, 63, 64, 65} <= {b for b, *_ in m.FPS_CASES}
    assert {1, 2, 127, 128, 129, 511, 512, 513, 1023, 1024, 1025, 3072, 3073} <= {n for _, n, _, _ in m.FPS_CASES}
    assert any(s == 1 for _, _, s, _ in m.FPS_CASES) and any(s == n for _, n, s, _ in m.FPS_CASES)
    assert any(s > n for _, n, s, _ in m.FPS_CASES) and any(c for *_, c in m.FPS_CASES)
    for n_edge in (128, 512, 1024):                                  # the wave kernels' limits from both sides, B >= 64
        assert any(b >= 64 and n == n_edge for b, n, _, _ in m.FPS_CASES)
        assert any(b >= 64 and n == n_edge + 1 for b, n, _, _ in m.FPS_CASES)
    assert {1, 16, 64, 128} <= {k for *_, k in m.BALL_CASES}
    assert {1, 127, 128, 1024, 1025, 4096} <= {n for _, n, _, _ in m.BALL_CASES}
