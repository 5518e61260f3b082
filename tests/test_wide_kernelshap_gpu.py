"""GPU: the wide regression (KernelSHAP) estimator - the three entry points of csrc/iq_kshap_wide.hip against the NumPy restatement
of the contract (tests/wide_kernelshap_ref.py) and, up to 64 regions, against their narrow twins bit for bit; the enumeration
identity against iq_exact_shapley; the stream contract against a host-only draw; the whole path through models; the driver.

Tolerances come from the number formats, not from measurements: the moment is held to the float64 bound of t terms in any order,
t 2^-53 sum|terms|; phi to the operation count of the closed form (``_phi_bound``); the enumerated game to one float32 rounding per
marginal plus the closed form's own n 2 H_{n-1} 2^-52.  No test is statistical."""
import argparse
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import probes
import wide_kernelshap_ref as ref
from interpret_quality_amd import _lib, final_common, hip_ops, kernelshap, synth, wide, wide_kernelshap

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


# ---- keep masks ----

def _orders_and_sizes(r, s, seed):
    """``s`` permutations of r regions and sizes in 1 .. r-1 that include 1, r-1 and, where they exist, 63, 64 and 65."""
    rng = np.random.default_rng(seed)
    orders = np.stack([rng.permutation(r) for _ in range(s)]).astype(np.int64)
    sizes = rng.integers(1, r, size=s)
    must = sorted({x for x in (1, r - 1, 63, 64, 65) if 1 <= x <= r - 1})
    sizes[:len(must)] = must
    return orders, sizes


@pytest.mark.parametrize("paired", [True, False])
@pytest.mark.parametrize("r", [2, 63, 64, 65, 128, 129, 1023, 1024])
def test_wide_keep_masks_are_bit_exact(r, paired):
    s, w = 37, (r + 63) // 64
    orders, sizes = _orders_and_sizes(r, s, 10 * r + paired)
    od, sd = hip_ops.as_i32(orders, DEV), hip_ops.as_i32(sizes, DEV)
    got = _u64(hip_ops.kshap_keep_masks_wide(od, sd, paired))
    want = ref.rows_from_orders(orders, sizes, r, paired)
    assert got.shape == ((2 * s if paired else s), w)
    assert np.array_equal(got, want), (r, paired)
    if r & 63:
        assert not np.any(got[:, -1] >> np.uint64(r & 63)), "a bit at or above R"
    assert np.array_equal(ref.bits(got[0::2] if paired else got, r).sum(axis=1), sizes)
    if paired:
        full = ref.full_row(r)
        assert np.array_equal(got[0::2] ^ got[1::2], np.broadcast_to(full, (s, w)))
        assert not np.any(got[0::2] & got[1::2])
    if r <= 64:
        assert np.array_equal(got[:, 0], _u64(hip_ops.kshap_keep_masks(od, sd, paired)))


@pytest.mark.parametrize("r", [2, 65, 1024])
def test_wide_keep_masks_refuse_a_size_of_0_or_r_and_an_entry_outside_the_game(r):
    orders = np.stack([np.arange(r)] * 3).astype(np.int64)
    good = np.array([1, 1, r - 1])
    for bad in (0, r, -1, r + 5):
        sizes = good.copy()
        sizes[1] = bad
        with pytest.raises(_lib.IqError, match="size"):
            hip_ops.kshap_keep_masks_wide(hip_ops.as_i32(orders, DEV), hip_ops.as_i32(sizes, DEV))
    for bad in (r, -1, 1 << 20):
        o = orders.copy()
        o[1, 0] = bad
        with pytest.raises(_lib.IqError, match="order entry"):
            hip_ops.kshap_keep_masks_wide(hip_ops.as_i32(o, DEV), hip_ops.as_i32(good, DEV), paired=False)
    # the rows the entry point itself leaves: the refused sample and its complement are 0, the others are written as usual
    lib, w = _lib.load(), (r + 63) // 64
    first_of_row_1 = (np.arange(3)[:, None] == 1) & (np.arange(r)[None] == 0)
    for sizes, o, verdict in ((np.array([1, 0, r - 1]), orders, 1), (np.array([1, r, r - 1]), orders, 1),
                              (good, np.where(first_of_row_1, -1, orders), 2), (good, np.where(first_of_row_1, r, orders), 2)):
        od, sd = hip_ops.as_i32(o, DEV), hip_ops.as_i32(sizes, DEV)
        keep = torch.full((6, w), -1, dtype=torch.int64, device=DEV)
        status = torch.zeros((1,), dtype=torch.int32, device=DEV)
        rc = lib.iq_kshap_keep_masks_wide(ctypes.c_void_p(od.data_ptr()), ctypes.c_void_p(sd.data_ptr()), ctypes.c_void_p(keep.data_ptr()),
                                          3, r, 1, ctypes.c_void_p(status.data_ptr()), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0 and int(status.item()) == verdict
        rows = _u64(keep)
        assert not rows[2:4].any(), "a refused row is written as 0"
        want = ref.rows_from_orders(orders[[0, 2]], [1, r - 1], r)
        assert np.array_equal(rows[[0, 1, 4, 5]], want)
    # the call after a refusal works
    got = _u64(hip_ops.kshap_keep_masks_wide(hip_ops.as_i32(orders, DEV), hip_ops.as_i32(good, DEV), paired=False))
    assert np.array_equal(got, ref.rows_from_orders(orders, good, r, paired=False))


# ---- moments ----

def _rows(rng, m, r):
    """Random wide rows; row 0 carries every bit at and above R as well (they are not looked at)."""
    w = (r + 63) // 64
    k = rng.integers(0, 1 << 63, size=(m, w), dtype=np.uint64) << np.uint64(1) | rng.integers(0, 2, size=(m, w), dtype=np.uint64)
    if r & 63:
        k[1:, -1] &= np.uint64((1 << (r & 63)) - 1)
    return k


def _within(got, want, bound, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = np.abs(got - want)
    print("%s: worst |got - want| / bound = %.3g" % (what, float((err / np.maximum(bound, 1e-300)).max())))
    assert np.all(err <= bound), what


@pytest.mark.parametrize("m", [1, 255, 256, 257, 65537])
@pytest.mark.parametrize("r", [2, 64, 65, 1024])
def test_wide_moment_matches_the_exact_sums_repeats_bitwise_and_is_the_narrow_moment_up_to_64_regions(r, m):
    """M = 65 537: 257 tiles, 2 per chunk, 129 chunks, the last one ragged (one tile holding one row)."""
    rng = np.random.default_rng(1000 * r + m)
    keep = _rows(rng, m, r)
    v = (rng.standard_normal((3, m)) * 3).astype(np.float32)
    v0 = rng.standard_normal(3)
    w = rng.uniform(0.01, 2.0, size=m)
    kt, vt, v0t, wt = hip_ops.wide_masks_to_tensor(keep, DEV), torch.from_numpy(v).to(DEV), torch.from_numpy(v0).to(DEV), torch.from_numpy(w).to(DEV)
    for weights, wdev in ((None, None), (w, wt)):
        tag = "R=%d M=%d %s" % (r, m, "weighted" if weights is not None else "unweighted")
        b3, w3 = hip_ops.kshap_moment_wide(kt, vt, v0t, r, wdev)
        assert b3.shape == (3, r) and w3.shape == (1,) and b3.dtype == torch.float64
        b3r, w3r = hip_ops.kshap_moment_wide(kt, vt, v0t, r, wdev)
        assert torch.equal(b3, b3r) and torch.equal(w3, w3r), tag + ": two calls"
        for g in range(3):
            b1, w1 = hip_ops.kshap_moment_wide(kt, vt[g:g + 1].contiguous(), v0t[g:g + 1].contiguous(), r, wdev)
            assert torch.equal(b1[0], b3[g]) and torch.equal(w1, w3), (tag, g)
        want_b, want_w = ref.moment(keep, v, v0, r, weights)
        _within(b3.cpu().numpy(), want_b, ref.moment_bound(keep, v, v0, r, weights), tag + " b")
        if weights is None:
            assert float(w3.item()) == float(m)
        else:
            assert abs(float(w3.item()) - want_w) <= m * ref.U * float(w.sum())
        if r <= 64:
            _, bn, wn = hip_ops.kshap_accum(kt[:, 0].contiguous(), vt, v0t, r, wdev)
            assert torch.equal(bn, b3) and torch.equal(wn, w3), tag + ": the narrow entry's bits"


# ---- phi ----

def _phi_bound(x, delta, r):
    """The closed form as the kernel evaluates it (include/iq.h), u = 2^-53, x = b / wsum, H = H_{R-1}: x_i carries one rounding
    (u |x_i|); y_i = x_i - c one more (u |y_i| <= 2 u max|x|); the error of c itself cancels in y_i - d, d being the mean of the
    y; d = sum(y) / R in index order carries at most (R - 1) u mean|y| + u |d| <= R u 2 mean|x|... all of it within
    (R + 4) u (max|x| + mean|x|) for the bracket, times 2 H (itself R roundings of a sum of positive terms: relative R u, inside
    the same count), plus the product's and the final sum's roundings and delta / R's: together the issue's
    (R + 4) 2^-53 (2 H (max|x| + mean|x|) + |delta| / R), taken as it stands."""
    h = ref.harmonic(r)
    return (r + 4) * ref.U * (2 * h * (np.abs(x).max() + np.abs(x).mean()) + abs(delta) / r)


@pytest.mark.parametrize("r", [2, 3, 64, 65, 128, 1023, 1024])
def test_phi_analytic_is_the_closed_form(r):
    rng = np.random.default_rng(r)
    wsum = 1000.5
    # game 0: unrelated values; game 1: the shape of real data, R nearly equal values whose differences carry phi; game 2: zeros
    b = np.stack([rng.standard_normal(r) * wsum, (0.25 + 1e-4 * rng.standard_normal(r)) * wsum, np.zeros(r)])
    delta = np.array([rng.standard_normal(), 0.5, -3.0])
    phi = hip_ops.kshap_phi_analytic(torch.from_numpy(b).to(DEV), torch.tensor([wsum], dtype=torch.float64, device=DEV),
                                     torch.from_numpy(delta).to(DEV)).cpu().numpy()
    assert phi.shape == (3, r) and phi.dtype == np.float64
    for g in range(3):
        want = ref.closed_form(b[g], wsum, delta[g], r)
        err = float(np.abs(phi[g].astype(ref.L) - want).max())
        bound = _phi_bound(b[g] / wsum, delta[g], r)
        total = math.fsum(phi[g])
        print("R=%d game %d: max |phi - closed form| = %.3g (bound %.3g), |sum(phi) - delta| = %.3g (bound %.3g)"
              % (r, g, err, bound, abs(total - delta[g]), r * 2.0 ** -52 * math.fsum(np.abs(phi[g]))))
        assert err <= bound
        assert abs(total - delta[g]) <= r * 2.0 ** -52 * math.fsum(np.abs(phi[g]))
    assert np.array_equal(phi[2], np.full(r, -3.0 / r))


def test_wide_estimate_at_64_regions_is_the_narrow_analytic_estimate():
    np.random.seed(64)
    keep, _ = kernelshap.draw(64, 4000, True, DEV)
    rng = np.random.default_rng(64)
    v = torch.from_numpy((rng.standard_normal((2, 4000)) * 3).astype(np.float32)).to(DEV)
    v_empty, v_full = [0.25, -1.0], [1.5, 2.0]
    narrow = kernelshap.estimate(keep, v, v_empty, v_full, 64, gram="analytic")
    got = wide_kernelshap.estimate(keep.reshape(-1, 1).contiguous(), v, v_empty, v_full, 64)
    assert got.shape == narrow.shape == (2, 64)
    for g in range(2):
        bound = 64 * ref.cond_analytic(64) * 2.0 ** -52 * float(np.abs(got[g]).max())
        print("game %d: max |wide - narrow| = %.3g (bound %.3g)" % (g, np.abs(got[g] - narrow[g]).max(), bound))
        assert np.abs(got[g] - narrow[g]).max() <= bound
    one = wide_kernelshap.estimate(keep.reshape(-1, 1).contiguous(), v[1].contiguous(), v_empty[1], v_full[1], 64)
    assert one.shape == (64,) and np.array_equal(one, got[1])


# ---- the enumeration identity on the device ----

@pytest.mark.parametrize("n", [2, 3, 10, 12])
def test_enumerated_game_through_the_wide_entries_is_exact_shapley(n):
    v = (np.random.default_rng(80 + n).standard_normal(1 << n) * 3).astype(np.float32)
    vt = torch.from_numpy(v).to(DEV)
    keep, weights = wide_kernelshap.enumerated(n, DEV)
    k, w = ref.enumerated(n)
    assert keep.shape == ((1 << n) - 2, 1) and np.array_equal(_u64(keep), k) and np.array_equal(weights.cpu().numpy(), w)
    phi = wide_kernelshap.estimate(keep, vt.index_select(0, keep[:, 0]).contiguous(), float(v[0]), float(v[-1]), n, weights)
    want = hip_ops.exact_shapley(vt).cpu().numpy()
    vmax = float(np.abs(v).max())
    bound = 2.0 ** -23 * vmax + n * 2 * ref.harmonic(n) * 2.0 ** -52 * vmax
    print("n=%d: max |phi - exact| / max|v| = %.3g (bound %.3g)" % (n, np.abs(phi - want).max() / vmax, bound / vmax))
    assert phi.shape == (n,) and phi.dtype == np.float64
    assert np.abs(phi - want).max() <= bound


# ---- the stream contract ----

@pytest.mark.parametrize("r", [65, 1024])
def test_draw_is_the_host_only_draw_whatever_the_chunk(r):
    s = 16
    np.random.seed(5)
    want_sizes, want_orders = ref.host_draw(r, s)
    host_after = np.random.get_state()
    want = ref.rows_from_orders(want_orders, want_sizes, r)
    for chunk in (1, 5, s, wide_kernelshap.DRAW_CHUNK):
        np.random.seed(5)
        keep, sizes = wide_kernelshap.draw(r, 2 * s, True, DEV, chunk=chunk)
        assert keep.shape == (2 * s, (r + 63) // 64) and keep.dtype == torch.int64
        assert np.array_equal(sizes, want_sizes) and np.array_equal(_u64(keep), want), (r, chunk)
        assert _same_state(np.random.get_state(), host_after), (r, chunk)
    np.random.seed(5)
    none, sizes = wide_kernelshap.draw(r, 2 * s, True, DEV, skip=True)
    assert none is None and np.array_equal(sizes, want_sizes) and _same_state(np.random.get_state(), host_after)
    np.random.seed(5)
    keep, sizes = wide_kernelshap.draw(r, s, False, DEV, chunk=5)
    assert np.array_equal(_u64(keep), ref.rows_from_orders(want_orders, want_sizes, r, paired=False))
    assert _same_state(np.random.get_state(), host_after)


def test_draw_at_64_regions_is_the_narrow_draw():
    np.random.seed(9)
    narrow, narrow_sizes = kernelshap.draw(64, 200, True, DEV)
    after = np.random.get_state()
    np.random.seed(9)
    keep, sizes = wide_kernelshap.draw(64, 200, True, DEV, chunk=7)
    assert keep.shape == (200, 1) and torch.equal(keep[:, 0], narrow) and np.array_equal(sizes, narrow_sizes)
    assert _same_state(np.random.get_state(), after)


# ---- through models ----

def _game(family, n, r):
    """Synthetic cloud 0 at its first n points, r regions from the device's own FPS (r = n: one region per point)."""
    pts, y = synth.make_cloud(0, n)
    data = torch.from_numpy(np.ascontiguousarray(pts))[None].to(DEV)
    fps = hip_ops.fps(data, r)[0].contiguous()
    rid = hip_ops.region_assign_wide(data[0].contiguous(), fps).cpu().numpy().astype(np.int64)
    args = argparse.Namespace(model=family, softmax_type="modified", num_points=n, num_regions=r, verbose=False)
    return data, torch.tensor([y], device=DEV), rid, args


def _through(family, n, r, samples, counts, coalitions=None):
    data, lbl, rid, args = _game(family, n, r)
    model, _ = probes.coalition_model(family, DEV)
    np.random.seed(31)
    phi, v_full, v_empty, running = wide_kernelshap.shapley(model, data, lbl, rid, args, samples=samples, counts=counts, coalitions=coalitions)
    after = np.random.get_state()
    np.random.seed(31)
    keep, _ = wide_kernelshap.draw(r, samples, True, DEV)
    assert _same_state(np.random.get_state(), after)
    v, f2, e2 = wide_kernelshap.rewards(model, data, lbl, rid, args, keep, coalitions)
    assert (f2, e2) == (v_full, v_empty) and v.shape == (samples,) and v.dtype == torch.float32
    # the rewards are the coalition entry's on the same rows, in one call and in ragged chunks
    ends = hip_ops.wide_masks_to_tensor(np.stack([ref.full_row(r), np.zeros_like(ref.full_row(r))]), DEV)
    with torch.no_grad():
        direct = final_common.get_reward(wide.coalition_logits(model, data, rid, torch.cat([keep, ends]), args, coalitions), lbl, args)
    assert torch.equal(direct[:-2], v) and float(direct[-2]) == v_full and float(direct[-1]) == v_empty
    v7, f7, e7 = wide_kernelshap.rewards(model, data, lbl, rid, args, keep, coalitions, chunk=7 + samples // 3)
    assert torch.equal(v7, v) and (f7, e7) == (v_full, v_empty)
    # phi is the restatement's on those rewards, and the running estimates are ``estimate`` on the row prefixes
    vh, rows = v.cpu().numpy(), _u64(keep)
    vmax = float(max(np.abs(vh).max(), abs(v_full), abs(v_empty)))
    want = ref.estimate(rows, vh, v_empty, v_full, r)
    print("%s N=%d R=%d %s: max |phi - restatement| / max|v| = %.3g" % (family, n, r, coalitions, np.abs(phi - want).max() / vmax))
    assert phi.shape == (r,) and phi.dtype == np.float64
    assert np.abs(phi - want).max() <= 1e-9 * vmax
    assert abs(math.fsum(phi) - (v_full - v_empty)) <= 1e-12 * vmax
    assert sorted(running) == [c for c in counts if c <= samples]
    for c, est in running.items():
        assert np.array_equal(est, wide_kernelshap.estimate(keep[:c].contiguous(), v[:c].contiguous(), v_empty, v_full, r)), c
        assert np.abs(est - ref.estimate(rows[:c], vh[:c], v_empty, v_full, r)).max() <= 1e-9 * vmax
    assert np.array_equal(running[samples], phi)
    return phi


@pytest.mark.parametrize("n,r,samples", [(256, 65, 600), (128, 128, 600), (1024, 1024, 64)])
def test_sampled_wide_game_through_pointnet(n, r, samples):
    _through("pointnet", n, r, samples, [10, samples // 2, samples, 10 * samples])


def test_sampled_wide_game_through_a_grouped_family_dense_and_compact():
    """PointNet++ at its smallest cloud (128 points), 65 regions: both ways of evaluating the coalitions, each held to the
    coalition entry's own rewards on the same rows."""
    for coalitions in ("dense", "compact"):
        _through("pointnet2", 128, 65, 200, [100, 200], coalitions)


# ---- driver ----

def _run_driver(cwd, extra):
    env = dict(os.environ, PYTHONPATH=REPO)
    cmd = [sys.executable, os.path.join(REPO, "final_wide_kernel_shapley.py"), "--model", "pointnet", "--dataset", "modelnet10", "--synthetic",
           "--num_clouds", "2", "--num_regions", "65", "--samples", "400"] + extra
    r = subprocess.run(cmd, cwd=str(cwd), env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


def test_final_wide_kernel_shapley_script_end_to_end(tmp_path, monkeypatch):
    """One child process writes both clouds; cloud 2 alone is then written in this process (the same ``main``, the cloud subset
    through the environment as every stage takes it): its files do not depend on whether cloud 1 was selected."""
    both = tmp_path / "both"
    both.mkdir()
    out = _run_driver(both, [])
    folder = "exp_MODEL_pointnet_DATA_modelnet10_POINTNUM_1024_REGIONNUM_65_shapley_test"
    seen = []
    for cloud in ("synthetic_00", "synthetic_01"):
        root = both / "checkpoints" / folder / cloud / "kernelshap"
        keep, v, phi = np.load(root / "coalitions.npy"), np.load(root / "rewards.npy"), np.load(root / "region_shapley_value.npy")
        counts, running = np.load(root / "running_counts.npy"), np.load(root / "running_region_shapley_value.npy")
        assert keep.shape == (400, 2) and keep.dtype == np.uint64
        assert v.shape == (400,) and v.dtype == np.float32
        assert phi.shape == (65,) and phi.dtype == np.float64
        assert counts.dtype == np.int64 and counts.ndim == 1 and running.shape == (len(counts), 65) and running.dtype == np.float64
        assert np.array_equal(keep[0::2] ^ keep[1::2], np.broadcast_to(ref.full_row(65), (200, 2)))
        line = [l for l in out.splitlines() if l.startswith("pointcloud:%s," % cloud)]
        assert len(line) == 1 and "sum(phi)=" in line[0] and "v_full - v_empty=" in line[0]
        delta = float(line[0].split("v_full - v_empty=")[1].split(",")[0])
        assert abs(math.fsum(phi) - delta) <= 1e-6 + 1e-12 * float(np.abs(v).max())      # the line prints six decimals
        assert len(counts) == 0                          # 400 rows are fewer than 100 permutations' worth of 66 evaluations
        seen.append(keep)
    assert not np.array_equal(seen[0], seen[1])          # the stream runs on from cloud to cloud
    from interpret_quality_amd import shapley_stage, wide_kernel_stage
    alone = tmp_path / "alone"
    alone.mkdir()
    monkeypatch.chdir(alone)
    args = wide_kernel_stage.make_args(["--model", "pointnet", "--dataset", "modelnet10", "--synthetic", "--num_clouds", "2",
                                        "--num_regions", "65", "--samples", "400"])
    shapley_stage.finish_args(args)
    args.cloud_subset = {1}
    wide_kernel_stage.run(args)
    for name in wide_kernel_stage.FILES:
        a = (both / "checkpoints" / folder / "synthetic_01" / "kernelshap" / (name + ".npy")).read_bytes()
        b = (alone / "checkpoints" / folder / "synthetic_01" / "kernelshap" / (name + ".npy")).read_bytes()
        assert a == b, name
    assert not (alone / "checkpoints" / folder / "synthetic_00" / "kernelshap").exists()
