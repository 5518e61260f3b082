"""GPU: the regression (KernelSHAP) estimator - the three entry points of csrc/iq_kshap.hip against the NumPy restatement of the
contract (tests/kernelshap_ref.py), the enumeration identity against iq_exact_shapley, the whole path through a model against
exact.shapley and the restatement, and the driver.

Tolerances come from the number formats, not from measurements: sums are held to the float64 bound of t terms in any order,
t 2^-53 sum|terms| (the bound of tests/test_exact_gpu.py); the solve to 4 x the residual of NumPy's own solution plus
n 2^-52 (|A| |phi| + |b|); the enumerated game to one float32 rounding per marginal plus n cond(A) 2^-52."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import kernelshap_ref as ref
import probes
from interpret_quality_amd import _lib, exact, hip_ops, kernelshap, synth

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


# ---- masks ----

@pytest.mark.parametrize("paired", [True, False])
@pytest.mark.parametrize("n", [2, 3, 31, 32, 33, 63, 64])
def test_keep_masks_are_bit_exact(n, paired):
    rng = np.random.default_rng(100 * n + paired)
    for s in (1, 64, 257):
        orders = np.stack([rng.permutation(n) for _ in range(s)]).astype(np.int64)
        sizes = rng.integers(1, n, size=s)
        sizes[0] = n - 1 if s == 1 and n % 2 else 1          # sizes 1 and n-1 are always among the cases
        sizes[-1] = sizes[-1] if s == 1 else n - 1
        got = _u64(hip_ops.kshap_keep_masks(hip_ops.as_i32(orders, DEV), hip_ops.as_i32(sizes, DEV), paired))
        want = ref.rows_from_orders(orders, sizes, n, paired)
        assert got.shape == (2 * s if paired else s,)
        assert np.array_equal(got, want), (n, s, paired)
        if n < 64:
            assert not np.any(got >> np.uint64(n)), "a bit at or above n"
        if paired:
            assert np.array_equal(got[0::2] ^ got[1::2], np.full(s, (1 << n) - 1, dtype=np.uint64))
            assert not np.any(got[0::2] & got[1::2])


@pytest.mark.parametrize("n", [2, 33, 64])
def test_keep_masks_refuse_a_size_of_0_or_n_and_an_entry_outside_the_game(n):
    orders = np.stack([np.arange(n)] * 3).astype(np.int64)
    for bad in (0, n, -1, n + 5):
        sizes = np.array([1, bad, n - 1])
        with pytest.raises(_lib.IqError, match="size"):
            hip_ops.kshap_keep_masks(hip_ops.as_i32(orders, DEV), hip_ops.as_i32(sizes, DEV))
    for bad in (n, -1, 64, 1 << 20):
        o = orders.copy()
        o[1, 0] = bad
        with pytest.raises(_lib.IqError, match="order entry"):
            hip_ops.kshap_keep_masks(hip_ops.as_i32(o, DEV), hip_ops.as_i32(np.array([1, 1, 1]), DEV), paired=False)
    # the call after a refusal works
    got = _u64(hip_ops.kshap_keep_masks(hip_ops.as_i32(orders, DEV), hip_ops.as_i32(np.array([1, 1, n - 1]), DEV), paired=False))
    assert got[0] == 1 and got[2] == (1 << (n - 1)) - 1


# ---- moments ----

def _masks(rng, m, n):
    k = rng.integers(0, 1 << 63, size=m, dtype=np.uint64) << np.uint64(1) | rng.integers(0, 2, size=m, dtype=np.uint64)
    return k if n == 64 else k & np.uint64((1 << n) - 1)


def _within(got, want, bound, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = np.abs(got - want)
    print("%s: worst |got - want| / bound = %.3g" % (what, float((err / np.maximum(bound, 1e-300)).max())))
    assert np.all(err <= bound), what


@pytest.mark.parametrize("m", [1, 2, 255, 256, 257, 4099])
@pytest.mark.parametrize("n", [2, 33, 64])
def test_moments_match_float64_numpy_and_repeat_bitwise(n, m):
    rng = np.random.default_rng(1000 * n + m)
    keep = _masks(rng, m, n)
    if n == 64 and m >= 2:
        keep[0] |= np.uint64((1 << 63) | (1 << 32) | (1 << 31))       # bits 31, 32 and 63 are ordinary bits
        keep[1] &= np.uint64(~((1 << 63) | (1 << 32) | (1 << 31)) & (2 ** 64 - 1))
    v = (rng.standard_normal((3, m)) * 3).astype(np.float32)
    v0 = rng.standard_normal(3)
    w = rng.uniform(0.01, 2.0, size=m)
    kt, vt, v0t, wt = hip_ops.masks_to_tensor(keep, DEV), torch.from_numpy(v).to(DEV), torch.from_numpy(v0).to(DEV), torch.from_numpy(w).to(DEV)
    for weights, wdev in ((None, None), (w, wt)):
        tag = "n=%d M=%d %s" % (n, m, "weighted" if weights is not None else "counts")
        a3, b3, w3 = hip_ops.kshap_accum(kt, vt, v0t, n, wdev)
        assert a3.shape == (n, n) and b3.shape == (3, n) and w3.shape == (1,)
        # two calls give the same bits, and G = 3 is three calls with G = 1
        a3r, b3r, w3r = hip_ops.kshap_accum(kt, vt, v0t, n, wdev)
        assert torch.equal(a3, a3r) and torch.equal(b3, b3r) and torch.equal(w3, w3r)
        for g in range(3):
            a1, b1, w1 = hip_ops.kshap_accum(kt, vt[g:g + 1].contiguous(), v0t[g:g + 1].contiguous(), n, wdev)
            assert torch.equal(a1, a3) and torch.equal(b1[0], b3[g]) and torch.equal(w1, w3), (tag, g)
            want_a, want_b, want_w = ref.moments(keep, v[g], v0[g], n, weights)
            bound_a, bound_b = ref.moment_bounds(keep, v[g], v0[g], n, weights)
            _within(b3[g].cpu().numpy(), want_b, bound_b, tag + " b[%d]" % g)
        if weights is None:
            assert np.array_equal(a3.cpu().numpy(), want_a), tag          # counts: exact
            assert float(w3.item()) == float(m)
        else:
            _within(a3.cpu().numpy(), want_a, bound_a, tag + " A")
            assert abs(float(w3.item()) - want_w) <= m * ref.U * float(w.sum())
        assert torch.equal(a3, a3.T)


# ---- solve ----

def _kkt_residual(a, b, delta, phi):
    """max(|A phi + lambda 1 - b|_inf with lambda from the first row, |sum(phi) - delta|), evaluated in extended precision."""
    L = np.longdouble
    ap = a.astype(L) @ phi.astype(L)
    lam = L(b[0]) - ap[0]
    return float(max(np.abs(ap + lam - b.astype(L)).max(), abs(phi.astype(L).sum() - L(delta))))


def _check_solve(a, b, delta, what):
    n = a.shape[0]
    phi = hip_ops.kshap_solve(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV), torch.from_numpy(delta).to(DEV)).cpu().numpy()
    assert phi.shape == b.shape
    for g in range(b.shape[0]):
        want, _ = ref.kkt_solve(a, b[g], delta[g])
        allow = 4 * _kkt_residual(a, b[g], delta[g], want) + n * 2.0 ** -52 * (
            np.abs(a).sum(axis=1).max() * np.abs(phi[g]).max() + np.abs(b[g]).max())
        got = _kkt_residual(a, b[g], delta[g], phi[g])
        print("%s g=%d: residual %.3g, allowed %.3g, max |phi - numpy| %.3g" % (what, g, got, allow, np.abs(phi[g] - want).max()))
        assert got <= allow, (what, g)
    return phi


@pytest.mark.parametrize("g", [1, 5])
@pytest.mark.parametrize("n", [2, 17, 64])
def test_solve_satisfies_the_kkt_system_as_well_as_numpy(n, g):
    np.random.seed(7 + n)
    sizes, orders = ref.host_draw(n, 20 * n)                       # 40 n paired rows
    keep = ref.rows_from_orders(orders, sizes, n)
    a, _, w = ref.moments(keep, np.zeros(len(keep)), 0.0, n)
    rng = np.random.default_rng(n + g)
    b, delta = rng.standard_normal((g, n)), rng.standard_normal(g)
    _check_solve(a / w, b, delta, "sampled n=%d G=%d" % (n, g))


def test_solve_of_the_analytic_gram_at_64_regions():
    rng = np.random.default_rng(64)
    _check_solve(kernelshap.analytic_gram(64), rng.standard_normal((3, 64)), rng.standard_normal(3), "analytic n=64")


@pytest.mark.parametrize("n", [2, 17, 64])
def test_rank_one_gram_is_a_status_word_not_a_fault(n):
    z = np.zeros(n)
    z[::2] = 1.0
    a = np.outer(z, z)                                             # all rows equal
    b, delta = torch.ones((2, n), dtype=torch.float64, device=DEV), torch.ones((2,), dtype=torch.float64, device=DEV)
    with pytest.raises(hip_ops.KshapSingular, match="do not determine the regression"):
        hip_ops.kshap_solve(torch.from_numpy(a).to(DEV), b, delta)
    with pytest.raises(_lib.IqError):
        hip_ops.kshap_solve(torch.zeros((n, n), dtype=torch.float64, device=DEV), b, delta)
    with pytest.raises(_lib.IqError):
        hip_ops.kshap_solve(torch.full((n, n), float("nan"), dtype=torch.float64, device=DEV), b, delta)
    # the process goes on: the next solve is a good one
    phi = hip_ops.kshap_solve(torch.eye(n, dtype=torch.float64, device=DEV), b, delta).cpu().numpy()
    assert np.abs(phi - 1.0 / n).max() <= 4 * n * ref.U            # x = 1, y = 1: phi = 1 - (n - 1) / n


# ---- the enumeration identity on the device ----

def _identity_bound(n, vmax):
    """One float32 rounding per marginal of at most 2 max|v| (iq_exact_shapley takes the marginals as the reference does), plus the
    float64 conditioning bound n cond(A) 2^-52 max|v|."""
    return 2.0 ** -23 * vmax + n * ref.cond_analytic(n) * 2.0 ** -52 * vmax


@pytest.mark.parametrize("n", [2, 3, 8, 12])
def test_enumerated_game_regresses_to_exact_shapley(n):
    v = (np.random.default_rng(50 + n).standard_normal(1 << n) * 3).astype(np.float32)
    vt = torch.from_numpy(v).to(DEV)
    keep, weights = kernelshap.enumerated(n, DEV)
    k, w = ref.enumerated(n)
    assert np.array_equal(_u64(keep), k) and np.array_equal(weights.cpu().numpy(), w)
    phi = kernelshap.estimate(keep, vt.index_select(0, keep).contiguous(), float(v[0]), float(v[-1]), n, weights)
    want = hip_ops.exact_shapley(vt).cpu().numpy()
    vmax = float(np.abs(v).max())
    print("n=%d: max |phi - exact| / max|v| = %.3g (bound %.3g)" % (n, np.abs(phi - want).max() / vmax, _identity_bound(n, vmax) / vmax))
    assert phi.shape == (n,) and phi.dtype == np.float64
    assert np.abs(phi - want).max() <= _identity_bound(n, vmax)
    assert np.array_equal(kernelshap.from_table(vt, keep, weights), phi)
    # the analytic A is the enumerated A: the same values up to the conditioning bound
    phi_a = kernelshap.from_table(vt, keep, weights, gram="analytic")
    assert np.abs(phi_a - phi).max() <= 2 * n * ref.cond_analytic(n) * 2.0 ** -52 * vmax + (1 << n) * ref.U * 2 * vmax * 2 * ref.cond_analytic(n)
    # G games on the same rows: row g is the single-game result, bit for bit
    v2 = torch.stack([vt.index_select(0, keep), 2 * vt.index_select(0, keep)]).contiguous()
    both = kernelshap.estimate(keep, v2, [float(v[0]), 2 * float(v[0])], [float(v[-1]), 2 * float(v[-1])], n, weights)
    assert both.shape == (2, n) and np.array_equal(both[0], phi)


# ---- through a model ----

R = 8
_CLOUDS = {}


def _cloud(family):
    """PointNet: synthetic cloud 0 at its 1024 points; PointNet++: its first 128 points.  Regions from the device's own FPS."""
    if family not in _CLOUDS:
        pts, y = synth.make_cloud(0)
        pts = pts[:128] if family == "pointnet2" else pts
        data = torch.from_numpy(np.ascontiguousarray(pts))[None].to(DEV)
        fps = hip_ops.fps(data, R)[0].contiguous()
        rid = hip_ops.region_assign(data[0].contiguous(), fps).cpu().numpy().astype(np.int64)
        args = argparse.Namespace(model=family, softmax_type="modified", num_points=data.shape[1], num_regions=R, verbose=False)
        _CLOUDS[family] = (data, torch.tensor([y], device=DEV), rid, args)
    return _CLOUDS[family]


@pytest.mark.parametrize("family", ["pointnet", "pointnet2"])
def test_enumerated_game_through_a_model_matches_exact_shapley(family):
    data, lbl, rid, args = _cloud(family)
    model, _ = probes.coalition_model(family, DEV)
    phi, v_full, v_empty, running = kernelshap.shapley(model, data, lbl, rid, args, samples="all")
    v = exact.value_table(model, data, lbl, rid, args)
    want, e_full, e_empty = exact.shapley(model, data, lbl, rid, args, v=v)
    vmax = float(v.abs().max())
    print("%s: max |phi - exact| / max|v| = %.3g" % (family, np.abs(phi - want).max() / vmax))
    assert (v_full, v_empty) == (e_full, e_empty) and running == {}
    assert np.abs(phi - want).max() <= _identity_bound(R, vmax)
    assert abs(phi.sum() - (v_full - v_empty)) <= 1e-12 * vmax


@pytest.mark.parametrize("family", ["pointnet", "pointnet2"])
def test_sampled_game_through_a_model_matches_the_restatement_and_the_stream_contract(family):
    data, lbl, rid, args = _cloud(family)
    model, _ = probes.coalition_model(family, DEV)
    np.random.seed(21)
    phi, v_full, v_empty, running = kernelshap.shapley(model, data, lbl, rid, args, samples=512, counts=[100, 257, 512, 4000])
    after = np.random.get_state()
    # the draw is reproducible, and it is the contract's: sizes from one random_sample call, then the permutations
    np.random.seed(21)
    keep, sizes = kernelshap.draw(R, 512, True, DEV)
    drawn = np.random.get_state()
    np.random.seed(21)
    keep2, _ = kernelshap.draw(R, 512, True, DEV)
    assert torch.equal(keep, keep2) and keep.shape == (512,)
    np.random.seed(21)
    want_sizes, want_orders = ref.host_draw(R, 256)
    host_after = np.random.get_state()
    assert np.array_equal(sizes, want_sizes)
    assert np.array_equal(_u64(keep), ref.rows_from_orders(want_orders, want_sizes, R))
    for got in (after, drawn):
        assert got[0] == host_after[0] and np.array_equal(got[1], host_after[1]) and got[2:] == host_after[2:]
    # the estimate is the restatement's on the same coalitions and the GPU's own rewards
    v, f2, e2 = kernelshap.rewards(model, data, lbl, rid, args, keep)
    assert (f2, e2) == (v_full, v_empty)
    vh = v.cpu().numpy()
    vmax = float(max(np.abs(vh).max(), abs(v_full), abs(v_empty)))
    want = ref.estimate(_u64(keep), vh, v_empty, v_full, R)
    print("%s: max |phi - restatement| / max|v| = %.3g" % (family, np.abs(phi - want).max() / vmax))
    assert np.abs(phi - want).max() <= 1e-9 * vmax
    assert abs(phi.sum() - (v_full - v_empty)) <= 1e-12 * vmax
    assert sorted(running) == [100, 256, 512] and np.array_equal(running[512], phi)
    for c in (100, 256):
        assert np.abs(running[c] - ref.estimate(_u64(keep)[:c], vh[:c], v_empty, v_full, R)).max() <= 1e-9 * vmax
    # the analytic variant on the same rows, and both read off the exact value table
    want_a = ref.estimate(_u64(keep), vh, v_empty, v_full, R, gram="analytic")
    got_a = kernelshap.estimate(keep, v, v_empty, v_full, R, gram="analytic")
    assert np.abs(got_a - want_a).max() <= 1e-9 * vmax
    table = exact.value_table(model, data, lbl, rid, args)
    assert torch.equal(table.index_select(0, keep), v)
    assert np.array_equal(kernelshap.from_table(table, keep), phi)


# ---- driver ----

def test_final_kernel_shapley_script_end_to_end(tmp_path):
    env = dict(os.environ, PYTHONPATH=REPO)
    cmd = [sys.executable, os.path.join(REPO, "final_kernel_shapley.py"), "--model", "pointnet", "--dataset", "modelnet10", "--synthetic",
           "--num_clouds", "2", "--num_regions", "8", "--samples", "512", "--compare_exact"]
    r = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    base = tmp_path / "checkpoints" / "exp_MODEL_pointnet_DATA_modelnet10_POINTNUM_1024_REGIONNUM_8_shapley_test"
    seen = []
    for cloud in ("synthetic_00", "synthetic_01"):
        root = base / cloud / "kernelshap"
        keep, v, phi = np.load(root / "coalitions.npy"), np.load(root / "rewards.npy"), np.load(root / "region_shapley_value.npy")
        counts, running = np.load(root / "running_counts.npy"), np.load(root / "running_region_shapley_value.npy")
        assert keep.shape == (512,) and keep.dtype == np.uint64
        assert v.shape == (512,) and v.dtype == np.float32
        assert phi.shape == (8,) and phi.dtype == np.float64
        assert counts.ndim == 1 and running.shape == (len(counts), 8) and running.dtype == np.float64
        assert np.array_equal(keep[0::2] ^ keep[1::2], np.full(256, 255, dtype=np.uint64))
        err = json.load(open(root / "sampling_error.json"))
        rows = err["sample_counts"]
        assert len(rows) >= 1 and {r_["evaluations"] for r_ in rows} >= {int(c) for c in counts}
        assert rows[-1]["samples"] == 512 // 9 and rows[-1]["kernelshap"]["rows"] == 504
        for row in rows:
            for est in ("permutation", "kernelshap"):
                assert row[est]["rms_error"] >= 0 and row[est]["max_abs_error"] >= row[est]["rms_error"]
        vmax = float(max(np.abs(v).max(), abs(err["v_full"]), abs(err["v_empty"])))
        assert abs(phi.sum() - (err["v_full"] - err["v_empty"])) <= 1e-12 * vmax
        assert err["final"]["rms_error"] >= 0 and err["num_regions"] == 8 and err["gram"] == "sampled" and err["paired"] is True
        line = [l for l in r.stdout.splitlines() if l.startswith("pointcloud:%s," % cloud)]
        assert len(line) == 1 and "rms error" in line[0]          # both estimators at the largest common budget
        seen.append(keep)
    assert not np.array_equal(seen[0], seen[1])          # the stream runs on from cloud to cloud


def test_driver_with_samples_all_writes_the_exact_values(tmp_path, monkeypatch):
    """--samples all: the enumerated game through the driver, in this process; its error against exact.shapley is the identity's."""
    from interpret_quality_amd import kernel_stage
    monkeypatch.chdir(tmp_path)
    kernel_stage.main(["--model", "pointnet", "--dataset", "modelnet10", "--synthetic", "--num_clouds", "1", "--num_regions", "8",
                       "--samples", "all", "--compare_exact"])
    root = tmp_path / "checkpoints" / "exp_MODEL_pointnet_DATA_modelnet10_POINTNUM_1024_REGIONNUM_8_shapley_test" / "synthetic_00" / "kernelshap"
    keep, v, phi = np.load(root / "coalitions.npy"), np.load(root / "rewards.npy"), np.load(root / "region_shapley_value.npy")
    assert np.array_equal(keep, np.arange(1, 255, dtype=np.uint64)) and v.shape == (254,) and phi.shape == (8,)
    assert np.load(root / "running_counts.npy").shape == (0,) and np.load(root / "running_region_shapley_value.npy").shape == (0, 8)
    err = json.load(open(root / "sampling_error.json"))
    vmax = float(max(np.abs(v).max(), abs(err["v_full"]), abs(err["v_empty"])))
    assert err["sample_counts"] == [] and err["final"]["max_abs_error"] <= _identity_bound(8, vmax)
    assert abs(phi.sum() - (err["v_full"] - err["v_empty"])) <= 1e-12 * vmax
