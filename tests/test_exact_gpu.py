"""GPU: exact games by full enumeration - the mask enumeration, the three lattice reductions against the brute-force reference
(tests/exact_ref.py), and the whole path (engines -> value table -> reductions) against the same quantities computed from the CPU
oracle's rewards.

Tolerance of the reductions: the float64 bound for a sum of t terms in any order, |got - want| <= t * 2^-53 * sum|terms| per
output (exact_ref returns it) - not a measured number."""
import argparse
import itertools
import json
import math

import numpy as np
import pytest
import torch

import exact_ref
import probes
from interpret_quality_amd import _lib, exact, hip_ops, synth

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _table(n, seed=0):
    return (np.random.default_rng(1000 * n + seed).standard_normal(1 << n) * 3).astype(np.float32)


def _within(got, want, bound, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    ratio = np.abs(got - want) / np.maximum(bound, 1e-300)
    worst = float(ratio.max()) if ratio.size else 0.0
    print("%s: worst |got - want| / bound = %.3g (max |err| %.3g)" % (what, worst, float(np.abs(got - want).max()) if ratio.size else 0.0))
    assert np.all(np.abs(got - want) <= bound), "%s: %.3g x the bound at %s" % (what, worst, np.unravel_index(ratio.argmax(), ratio.shape))


# ---- check 4: enumeration ----

def _enum_ref(first, count, n, players, base):
    c = (np.uint64(first) + np.arange(count, dtype=np.uint64))
    keep = np.full(count, base, dtype=np.uint64)
    for k in range(n):
        keep |= ((c >> np.uint64(k)) & np.uint64(1)) << np.uint64(players[k] if players is not None else k)
    return keep


@pytest.mark.parametrize("first,count,n,players,base", [
    (0, 256, 8, None, 0),
    (0, 2, 1, None, 0),
    (0, 2, 1, [63], 0b110),
    (5, 1000, 13, [12, 0, 7, 3, 31, 5, 9, 1, 2, 30, 11, 4, 8], (1 << 40) | (1 << 6)),
    (0, 1 << 16, 24, None, 0),
    ((1 << 24) - 4096, 4096, 24, list(range(23, -1, -1)), 1 << 50),
    ((1 << 32) - 100, 300, 24, None, 1 << 63),             # first > 2^32 - count: 64-bit index arithmetic
    ((1 << 40) + 12345, 777, 6, [5, 3, 1, 0, 2, 4], 1 << 7),
])
def test_enum_keep_masks_is_bit_exact(first, count, n, players, base):
    got = hip_ops.enum_keep_masks(first, count, n, DEV, players, base).cpu().numpy().view(np.uint64)
    assert np.array_equal(got, _enum_ref(first, count, n, players, base))


def test_enum_keep_masks_refuses_a_repeated_player_and_a_player_in_base():
    with pytest.raises(_lib.IqError, match="two players"):
        hip_ops.enum_keep_masks(0, 8, 3, DEV, [4, 2, 4], 0)
    with pytest.raises(_lib.IqError, match="base"):
        hip_ops.enum_keep_masks(0, 8, 3, DEV, [4, 2, 1], 0b100)
    with pytest.raises(_lib.IqError, match="base"):
        hip_ops.enum_keep_masks(0, 8, 3, DEV, None, 0b1)


# ---- check 5: the reductions ----

@pytest.mark.parametrize("n", [1, 2, 3, 8, 13, 20])
def test_reductions_match_the_brute_force_within_the_float64_bound_and_repeat_bitwise(n):
    v = _table(n)
    vt = torch.from_numpy(v).to(DEV)
    pairs = hip_ops.all_pairs(n)
    phi, inter, a = hip_ops.exact_shapley(vt), hip_ops.exact_interactions(vt), hip_ops.moebius(vt)
    assert inter.shape == (n * (n - 1) // 2, n - 1) and phi.shape == (n,) and a.shape == (1 << n,)
    # two calls give the same bits (other work in between: the scratch is a fresh allocation each time)
    assert torch.equal(phi, hip_ops.exact_shapley(vt)) and torch.equal(inter, hip_ops.exact_interactions(vt))
    assert torch.equal(a, hip_ops.moebius(vt))
    if n <= 13:
        want_phi, b_phi = exact_ref.shapley(v, n, with_bound=True)
        want_i, b_i = exact_ref.interactions(v, n, [tuple(p) for p in pairs], with_bound=True)
        want_a, b_a = exact_ref.dividends(v, n, with_bound=True)
    else:
        want_phi, b_phi = exact_ref.shapley_vectorised(v, n)
        want_i, b_i = exact_ref.interactions_vectorised(v, n, pairs)
        want_a, b_a = exact_ref.dividends_vectorised(v, n)
    _within(phi.cpu().numpy(), want_phi, b_phi, "phi n=%d" % n)
    _within(inter.cpu().numpy(), want_i, b_i, "interactions n=%d" % n)
    _within(a.cpu().numpy(), want_a, b_a, "dividends n=%d" % n)
    # a subset of the pairs, in another order, gives the same bits per pair (the order depends on n only)
    if n >= 3:
        sel = [len(pairs) - 1, 0, 1]
        sub = hip_ops.exact_interactions(vt, pairs[sel])
        assert torch.equal(sub, inter[sel])
    # (j, i) takes the two subtractions of the float32 term in the other order: held to the brute force of (j, i)
    if 3 <= n <= 13:
        rev = [(int(j), int(i)) for i, j in pairs[[0, 1, len(pairs) - 1]]]
        _within(hip_ops.exact_interactions(vt, rev).cpu().numpy(), *exact_ref.interactions(v, n, rev, with_bound=True), "reversed pairs n=%d" % n)


def test_bad_pairs_are_refused():
    vt = torch.from_numpy(_table(4)).to(DEV)
    with pytest.raises(_lib.IqError):
        hip_ops.exact_interactions(vt, [(0, 4)])
    with pytest.raises(_lib.IqError):
        hip_ops.exact_interactions(vt, [(2, 2)])
    with pytest.raises(_lib.IqError):
        hip_ops.exact_interactions(vt, torch.tensor([[1, 1]], device=DEV))


def test_exact_shapley_equals_shapley_accum_over_all_120_permutations():
    """Ties the new kernel to the existing, reference-pinned one: iq_shapley_accum fed with the prefix rewards of ALL 5!
    permutations has the exact value as its mean."""
    n = 5
    v = _table(n, 7)
    vt = torch.from_numpy(v).to(DEV)
    orders = np.array(list(itertools.permutations(range(n))), dtype=np.int64)
    snaps, rows = exact.sampled_from_table(vt, orders, [len(orders)])
    mean = snaps[len(orders)] / len(orders)
    _, b_phi = exact_ref.shapley(v, n, with_bound=True)
    b_mean = len(orders) * exact_ref.U * np.abs(rows).sum(axis=0) / len(orders)      # 120 terms of |row| / 120 per player
    _within(mean, hip_ops.exact_shapley(vt).cpu().numpy(), b_phi + b_mean, "mean of 120 permutations")
    assert np.array_equal(rows, exact_ref.sampled_rows(v, orders))


def _check_moebius_identities(v, n, phi, inter, a, pairs, what):
    """phi_k = sum over {c with k} of a[c] / |c|, and the interaction term of context S = sum of a[T + {i,j}] over T in S - on
    the device results.  The identities hold for exact differences; the kernels take them in float32 as the reference does, so
    each marginal carries one float32 rounding (2^-24 of at most 2 max|v|) and each interaction term three (9 * 2^-24 max|v|)."""
    vmax = float(np.abs(v).max())
    pc = exact_ref._popcounts(n)
    a_bound = exact_ref.dividends_vectorised(v, n)[1]              # 2^|c| 2^-53 sum over subsets t of c of |v[t]|
    idx = np.arange(1 << n)
    for k in range(n):
        has = ((idx >> k) & 1) == 1
        got = math.fsum(a[has] / pc[has])
        slack = 2.0 ** -23 * vmax + 2 * float((a_bound[has] / pc[has]).sum()) + (1 << (n - 1)) * exact_ref.U * 2 * vmax
        assert abs(got - phi[k]) <= slack, (what, k, got, phi[k], slack)
    # mean over the contexts of order m of the per-context identity = the kernel's out[p][m]
    for p in ([0, len(pairs) // 2, len(pairs) - 1] if len(pairs) else []):
        i, j = (int(x) for x in pairs[p])
        bij = (1 << i) | (1 << j)
        z = np.where((idx & bij) == bij, a, 0.0)      # zeta transform restricted to the supersets of {i,j}
        zb = np.where((idx & bij) == bij, a_bound, 0.0)
        for b in range(n):
            if b in (i, j):
                continue
            z = z.reshape(-1, 2, 1 << b)
            z[:, 1, :] += z[:, 0, :]
            zb = zb.reshape(-1, 2, 1 << b)
            zb[:, 1, :] += zb[:, 0, :]
            z, zb = z.reshape(-1), zb.reshape(-1)
        ctx = idx[(idx & bij) == 0]
        for m in range(n - 1):
            sel = ctx[pc[ctx] == m]
            got = math.fsum(z[sel | bij]) / len(sel)
            slack = 9 * 2.0 ** -24 * vmax + float(zb[sel | bij].sum()) / len(sel) * (n + 1) + len(sel) * exact_ref.U * 4 * vmax
            assert abs(got - inter[p, m]) <= slack, (what, p, m, got, inter[p, m], slack)


@pytest.mark.parametrize("n", [2, 8, 13])
def test_moebius_identities_hold_on_the_device_results(n):
    v = _table(n, 3)
    vt = torch.from_numpy(v).to(DEV)
    pairs = hip_ops.all_pairs(n)
    _check_moebius_identities(v, n, hip_ops.exact_shapley(vt).cpu().numpy(), hip_ops.exact_interactions(vt).cpu().numpy(),
                              hip_ops.moebius(vt).cpu().numpy(), pairs, "n=%d" % n)


# ---- checks 6-8: end to end ----

R = 8


def _args(family, num_regions=R):
    return argparse.Namespace(model=family, softmax_type="modified", num_points=1024, num_regions=num_regions, verbose=False)


_SETUP = {}


def _setup():
    if not _SETUP:
        data, lbl, rid = exact_ref.oracle_setup(R)
        _SETUP["x"] = (data, lbl, rid)
    return _SETUP["x"]


@pytest.mark.parametrize("family", ["pointnet", "pointnet2", "gcnn", "pointconv"])
def test_exact_values_from_the_hip_path_match_the_oracle(family):
    """R = 8: exact phi and all 28 x 7 interactions from the HIP path against exact_ref on the ORACLE's rewards of the 256 masked
    clouds.  Bars: phi 1e-4 relative norm-wise; element-wise |d phi|, |d I| <= 1e-4 * max|v|."""
    data, lbl, rid = _setup()
    model, sd = probes.coalition_model(family, DEV)
    args = _args(family)
    v = exact.value_table(model, data.to(DEV), lbl.to(DEV), rid, args)
    phi, v_full, v_empty = exact.shapley(model, data.to(DEV), lbl.to(DEV), rid, args, v=v)
    inter = exact.interactions(model, data.to(DEV), lbl.to(DEV), rid, args, v=v)
    ov = exact_ref.oracle_value_table(family, sd, data, lbl, rid, R)
    pairs = [tuple(p) for p in hip_ops.all_pairs(R)]
    o_phi, o_inter = exact_ref.shapley(ov, R), exact_ref.interactions(ov, R, pairs)
    vmax = float(np.abs(ov).max())
    rel = np.linalg.norm(phi - o_phi) / np.linalg.norm(o_phi)
    print("%s: phi rel %.3g, max |d phi| / max|v| %.3g, max |d I| / max|v| %.3g, table max |dv| / max|v| %.3g" % (
        family, rel, np.abs(phi - o_phi).max() / vmax, np.abs(inter - o_inter).max() / vmax, np.abs(v.cpu().numpy() - ov).max() / vmax))
    assert inter.shape == (28, 7)
    assert rel <= 1e-4
    assert np.abs(phi - o_phi).max() <= 1e-4 * vmax
    assert np.abs(inter - o_inter).max() <= 1e-4 * vmax
    assert v_full == float(v[-1]) and v_empty == float(v[0])
    assert abs(phi.sum() - (v_full - v_empty)) <= R * 2.0 ** -23 * vmax


def test_dgcnn_exact_values_satisfy_efficiency_and_the_moebius_identities():
    """DGCNN's parity bar against the oracle is qualified (dynamic graphs), so its exact values are held to what needs no
    reference: efficiency and both Moebius identities."""
    data, lbl, rid = _setup()
    model, _ = probes.coalition_model("dgcnn", DEV)
    args = _args("dgcnn")
    d, l = data.to(DEV), lbl.to(DEV)
    v = exact.value_table(model, d, l, rid, args)
    phi, v_full, v_empty = exact.shapley(model, d, l, rid, args, v=v)
    vh = v.cpu().numpy()
    assert abs(phi.sum() - (v_full - v_empty)) <= R * 2.0 ** -23 * float(np.abs(vh).max())
    _check_moebius_identities(vh, R, phi, exact.interactions(model, d, l, rid, args, v=v), exact.dividends(model, d, l, rid, args, v=v),
                              hip_ops.all_pairs(R), "dgcnn")


def test_stage1_sampled_estimate_is_within_5_standard_errors_of_the_exact_value():
    """PointNet: shapley_all_orders (stage 1) with the 1000 permutations of synth.make_orders(1000, 8, seed=1) lies within 5
    standard errors (from region_sv_all) of the exact phi for every region."""
    from interpret_quality_amd import shapley_stage
    data, lbl, rid = _setup()
    model, _ = probes.coalition_model("pointnet", DEV)
    args = _args("pointnet")
    args.shapley_batch_size = 1
    d, l = data.to(DEV), lbl.to(DEV)
    phi, _, _ = exact.shapley(model, d, l, rid, args)
    orders = synth.make_orders(1000, R, seed=1)
    snaps, region_sv_all, total = shapley_stage.shapley_all_orders(model, d, l, rid, orders, args)
    rms = {}
    for s in (100, 1000):
        est, se = snaps[s] / s, region_sv_all[:s].std(axis=0, ddof=1) / math.sqrt(s)
        z = np.abs((est - phi) / se)
        rms[s] = float(np.sqrt(((est - phi) ** 2).mean()))
        print("samples %d: max |z| %.2f, rms error %.4f" % (s, z.max(), rms[s]))
        assert z.max() < 5, (s, z)
    assert rms[1000] < rms[100]
    # the same estimate read off the value table (what final_exact_shapley.py reports) is stage 1's, bit for bit
    v = exact.value_table(model, d, l, rid, args)
    snaps_t, rows_t = exact.sampled_from_table(v, orders, [100, 1000])
    assert np.array_equal(rows_t, region_sv_all) and np.array_equal(snaps_t[1000], snaps[1000])


@pytest.mark.parametrize("family", ["pointnet", "pointnet2"])
def test_value_table_does_not_depend_on_chunk_and_equals_the_direct_calls(family):
    from interpret_quality_amd import final_common
    data, lbl, rid = _setup()
    model, _ = probes.coalition_model(family, DEV)
    args = _args(family)
    d, l = data.to(DEV), lbl.to(DEV)
    big = exact.value_table(model, d, l, rid, args, chunk=1 << 16)
    assert torch.equal(big, exact.value_table(model, d, l, rid, args, chunk=64))      # 256 coalitions in four steps
    # chunks of 2^10 against 2^16 on a table they split differently: 12 regions, 4096 coalitions
    data12, lbl12, rid12 = exact_ref.oracle_setup(12)
    a12 = _args(family, 12)
    assert torch.equal(exact.value_table(model, data12.to(DEV), lbl12.to(DEV), rid12, a12, chunk=1 << 10),
                       exact.value_table(model, data12.to(DEV), lbl12.to(DEV), rid12, a12, chunk=1 << 16))
    keep = hip_ops.masks_to_tensor(np.arange(1 << R, dtype=np.uint64), DEV)
    ridt = hip_ops.region_ids(rid, DEV, R).reshape(1, -1)
    logits = model.coalition_logits(d.contiguous(), torch.mean(d, dim=1).reshape(1, 3).contiguous(), ridt, keep, None, num_regions=R)
    assert torch.equal(big, final_common.get_reward(logits, l, args))
    # a game among 6 of the 8 regions, region 6 always kept, region 1 always masked: the full table at the matching indices
    players, base = [7, 0, 5, 2, 4, 3], 1 << 6
    sub = exact.value_table(model, d, l, rid, args, players=players, base=base).cpu().numpy()
    full = big.cpu().numpy()
    want = np.array([full[int(_enum_ref(c, 1, 6, players, base)[0])] for c in range(64)], dtype=np.float32)
    assert np.array_equal(sub, want)
    phi6, _, _ = exact.shapley(model, d, l, rid, args, players=players, base=base)
    want6, b6 = exact_ref.shapley(want, 6, with_bound=True)
    _within(phi6, want6, b6, "6-player game")
    with pytest.raises(_lib.IqError):
        exact.value_table(model, d, l, rid, args, players=[0, 1], base=0b10)


def test_pointnet_16_regions_efficiency_and_phi_from_dividends():
    n = 16
    data, lbl, rid = exact_ref.oracle_setup(n)
    model, _ = probes.coalition_model("pointnet", DEV)
    args = _args("pointnet", n)
    d, l = data.to(DEV), lbl.to(DEV)
    v = exact.value_table(model, d, l, rid, args)
    phi, v_full, v_empty = exact.shapley(model, d, l, rid, args, v=v)
    vh = v.cpu().numpy()
    assert vh.shape == (1 << n,) and np.isfinite(vh).all()
    want, bound = exact_ref.shapley_vectorised(vh, n)
    _within(phi, want, bound, "phi n=16")
    # efficiency: exact for exact differences; the float32 marginals carry one rounding each (2^-24 of at most 2 max|v|)
    assert abs(phi.sum() - (v_full - v_empty)) <= n * 2.0 ** -23 * float(np.abs(vh).max())
    _check_moebius_identities(vh, n, phi, exact.interactions(model, d, l, rid, args, v=v), exact.dividends(model, d, l, rid, args, v=v),
                              hip_ops.all_pairs(n), "pointnet n=16")


def test_final_exact_shapley_script_end_to_end(tmp_path, monkeypatch):
    from interpret_quality_amd import exact_stage
    monkeypatch.chdir(tmp_path)
    exact_stage.main(["--model", "pointnet", "--dataset", "modelnet10", "--synthetic", "--num_clouds", "1", "--num_regions", "8"])
    root = tmp_path / "checkpoints" / "exp_MODEL_pointnet_DATA_modelnet10_POINTNUM_1024_REGIONNUM_8_shapley_test" / "synthetic_00" / "exact"
    phi = np.load(root / "region_shapley_value.npy")
    inter = np.load(root / "interaction_all_orders.npy")
    v = np.load(root / "value_table.npy")
    assert phi.shape == (8,) and phi.dtype == np.float64
    assert inter.shape == (28, 7) and inter.dtype == np.float64
    assert v.shape == (256,) and v.dtype == np.float32
    _within(phi, *exact_ref.shapley(v, 8, with_bound=True), "script phi")
    err = json.load(open(root / "sampling_error.json"))["sample_counts"]
    assert [e["samples"] for e in err] == [100, 200, 300, 400, 500, 600, 700, 800, 900, 1000]
    assert err[-1]["rms_error"] < err[0]["rms_error"]
    assert all(e["max_abs_error_in_se"] < 5 for e in err)
