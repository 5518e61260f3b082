"""GPU: the all-pairs interaction estimator (SHAP-IQ on the regression rows; csrc/iq_kshap_pairs.hip) against the NumPy restatement
of its defining formula (tests/kshap_pairs_ref.py), its bits (two calls, G games, a game beside NaN rewards, narrow against wide
rows), the enumeration identity against iq_exact_interactions, the whole path through models, and both drivers' --pairs.

The tolerance is ``ref.bound``, (M + 16) 2^-53 sum |d| (|alpha| + 2 |beta| + |gamma|) / W_sum: the float64 worst case of the
alpha/beta/gamma form under any summation order - derived, not measured.  The enumeration identity adds 9 2^-24 max|v| for the
three float32 roundings of iq_exact_interactions' association (partial sums of at most 2, 3 and 4 max|v|); on an integer-valued
table those are exact and the bound stands alone.  No test is statistical."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import kshap_pairs_ref as ref
import probes
import wide_kernelshap_ref as wide_ref
from interpret_quality_amd import exact, hip_ops, kernelshap, synth, wide_kernelshap

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

REGIONS = [2, 3, 15, 16, 17, 63, 64, 65, 127, 128, 129, 1000, 1024]
ROWS = [1, 3, 4, 5, 255, 256, 257, 4097]
CASES = [(r, m) for r in REGIONS for m in ROWS] + [(r, 65537) for r in REGIONS if r <= 129]      # 65 537: several chunks


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _rows(r, m, rng):
    """M rows: random ones of the size law, each followed by its complement, and - where M has room - the hand-made rows of
    sizes 0, 1, 2, R-2, R-1 and R at the end (the last tile is the ragged one)."""
    edge = ref.edge_rows(r)
    keep = ref.size_law_rows(r, (m + 1) // 2, rng)[:m]
    if m >= 2 * len(edge):
        keep[-len(edge):] = edge
    return keep


def _device_rows(keep, r):
    """The rows on the device; row 0 also carries every bit at and above R (they are not looked at)."""
    k = keep.copy()
    if r & 63:
        k[0, -1] |= ~np.uint64((1 << (r & 63)) - 1)
    return hip_ops.wide_masks_to_tensor(k, DEV)


def _check(got, want, bound, what):
    err = float(np.abs(got - want).max())
    print("%s: max |got - restatement| = %.3g, bound %.3g, fraction %.3g" % (what, err, bound, err / bound if bound > 0 else 0.0))
    assert got.shape == want.shape and got.dtype == np.float64
    assert err <= bound, what
    assert not np.diag(got).any(), what + ": diagonal"
    assert np.array_equal(got, got.T), what + ": out[i][j] and out[j][i] differ"


@pytest.mark.parametrize("r,m", CASES)
def test_pairs_match_the_restatement_and_repeat_bitwise(r, m):
    rng = np.random.RandomState(1000 * r + m)
    keep = _rows(r, m, rng)
    v = (rng.standard_normal((3, m)) * 3).astype(np.float32)
    v0, delta = rng.standard_normal(3), rng.standard_normal(3)
    w = rng.uniform(0.01, 2.0, size=m)
    kt, vt, v0t, dt, wt = (_device_rows(keep, r), torch.from_numpy(v).to(DEV), torch.from_numpy(v0).to(DEV), torch.from_numpy(delta).to(DEV),
                           torch.from_numpy(w).to(DEV))
    tag = "R=%d M=%d" % (r, m)
    for game, weights, wdev in ((0, None, None), (1, w, wt)):
        out = hip_ops.kshap_pairs(kt, vt, v0t, dt, r, wdev)
        assert out.shape == (3, r, r) and out.dtype == torch.float64
        assert torch.equal(out, hip_ops.kshap_pairs(kt, vt, v0t, dt, r, wdev)), tag + ": two calls"
        for g in range(3):                                           # a game's bits depend neither on G nor on its place
            one = hip_ops.kshap_pairs(kt, vt[g:g + 1].contiguous(), v0t[g:g + 1].contiguous(), dt[g:g + 1].contiguous(), r, wdev)
            assert torch.equal(one[0], out[g]), (tag, g)
        want = ref.pairs(keep, v[game], v0[game], delta[game], r, weights)
        _check(out[game].cpu().numpy(), want, ref.bound(keep, v[game], v0[game], r, weights),
               "%s %s" % (tag, "weighted" if weights is not None else "unweighted"))
    poisoned = vt.clone()
    poisoned[1] = float("nan")                                        # the games never meet
    got = hip_ops.kshap_pairs(kt, poisoned, v0t, dt, r, None)
    clean = hip_ops.kshap_pairs(kt, vt, v0t, dt, r, None)
    assert torch.equal(got[0], clean[0]) and torch.equal(got[2], clean[2]), tag + ": a game beside NaN rewards"
    assert bool(torch.isnan(got[1]).any())


@pytest.mark.parametrize("r", [2, 3, 64, 65, 1024])
def test_rows_of_size_0_and_r_alone_return_the_share_of_delta(r):
    full, empty = wide_ref.full_row(r), np.zeros_like(wide_ref.full_row(r))
    keep = np.array([full, empty, empty, full, full], dtype=np.uint64).reshape(5, -1)
    v = torch.tensor([[3.0, -2.0, 7.0, 1.0, float("inf")]], dtype=torch.float32, device=DEV)
    out = hip_ops.kshap_pairs(_device_rows(keep, r), v, torch.tensor([0.5], dtype=torch.float64, device=DEV),
                              torch.tensor([4.0], dtype=torch.float64, device=DEV), r)[0].cpu().numpy()
    want = np.full((r, r), 4.0 / (r - 1))
    np.fill_diagonal(want, 0.0)
    assert np.array_equal(out, want)


@pytest.mark.parametrize("r", [2, 64])
def test_narrow_rows_and_the_same_rows_as_wide_give_the_same_bits(r):
    rng = np.random.RandomState(r)
    keep = _rows(r, 700, rng)
    v = torch.from_numpy((rng.standard_normal((2, 700)) * 3).astype(np.float32)).to(DEV)
    v0, delta = torch.from_numpy(rng.standard_normal(2)).to(DEV), torch.from_numpy(rng.standard_normal(2)).to(DEV)
    w = torch.from_numpy(rng.uniform(0.01, 2.0, size=700)).to(DEV)
    kt = hip_ops.wide_masks_to_tensor(keep, DEV)
    assert kt.shape == (700, 1)
    for weights in (None, w):
        assert torch.equal(hip_ops.kshap_pairs(kt[:, 0].contiguous(), v, v0, delta, r, weights), hip_ops.kshap_pairs(kt, v, v0, delta, r, weights))
    narrow = kernelshap.pairs(kt[:, 0].contiguous(), v[0].contiguous(), float(v0[0]), float(v0[0]) + float(delta[0]), r)
    assert narrow.shape == (r, r)


# ---- the enumeration identity on the device ----

def _exact_sii(vt, n):
    """(n,n): the mean over the orders of iq_exact_interactions' context-averaged I_ij^(m), all pairs."""
    pr = hip_ops.all_pairs(n)
    out = np.zeros((n, n))
    out[pr[:, 0], pr[:, 1]] = out[pr[:, 1], pr[:, 0]] = hip_ops.exact_interactions(vt).cpu().numpy().mean(axis=1)
    return out


def _identity(n, v, wide_rows, extra):
    vt = torch.from_numpy(v).to(DEV)
    if wide_rows:
        keep, weights = wide_kernelshap.enumerated(n, DEV)
        got = wide_kernelshap.pairs(keep, vt.index_select(0, keep[:, 0]).contiguous(), float(v[0]), float(v[-1]), n, weights)
    else:
        keep, weights = kernelshap.enumerated(n, DEV)
        got = kernelshap.pairs_from_table(vt, keep, weights)
    want = _exact_sii(vt, n)
    rows = _u64(keep).reshape(len(keep), -1)
    bound = ref.bound(rows, v[rows[:, 0].astype(np.int64)], float(v[0]), n, weights.cpu().numpy())
    vmax = float(np.abs(v).max())
    err = float(np.abs(got - want).max())
    print("n=%d %s: max |pairs - exact| = %.3g, bound %.3g + %.3g" % (n, "wide" if wide_rows else "narrow", err, bound, extra * vmax))
    assert got.shape == (n, n) and err <= extra * vmax + bound
    assert np.array_equal(got, got.T) and not np.diag(got).any()


@pytest.mark.parametrize("n", [2, 3, 8, 12])
def test_enumerated_rows_give_the_exact_index(n):
    _identity(n, (np.random.default_rng(90 + n).standard_normal(1 << n) * 3).astype(np.float32), False, 9 * 2.0 ** -24)
    _identity(n, np.random.default_rng(190 + n).integers(-40, 41, size=1 << n).astype(np.float32), False, 0.0)


@pytest.mark.parametrize("n", range(2, 13))
def test_enumerated_rows_through_the_wide_rows_give_the_exact_index(n):
    _identity(n, (np.random.default_rng(290 + n).standard_normal(1 << n) * 3).astype(np.float32), True, 9 * 2.0 ** -24)
    _identity(n, np.random.default_rng(390 + n).integers(-40, 41, size=1 << n).astype(np.float32), True, 0.0)


# ---- through models ----

def _game(family, n, r):
    """Synthetic cloud 0 at its first n points, r regions from the device's own FPS (r = n: one region per point)."""
    pts, y = synth.make_cloud(0, n)
    data = torch.from_numpy(np.ascontiguousarray(pts))[None].to(DEV)
    fps = hip_ops.fps(data, r)[0].contiguous()
    rid = hip_ops.region_assign_wide(data[0].contiguous(), fps).cpu().numpy().astype(np.int64)
    args = argparse.Namespace(model=family, softmax_type="modified", num_points=n, num_regions=r, verbose=False)
    return data, torch.tensor([y], device=DEV), rid, args


def _sampled(g, r, what):
    """A sampled game's interaction against the restatement on the game's own rows and rewards, within ``bound``."""
    assert g["weights"] is None and g["interaction"].shape == (r, r)
    keep, v = _u64(g["keep"]).reshape(len(g["keep"]), -1), g["v"].cpu().numpy()
    want = ref.pairs(keep, v, g["v_empty"], g["v_full"] - g["v_empty"], r)
    _check(g["interaction"], want, ref.bound(keep, v, g["v_empty"], r), what)
    assert np.array_equal(g["interaction"], (wide_kernelshap if g["keep"].dim() == 2 else kernelshap).pairs(
        g["keep"], g["v"], g["v_empty"], g["v_full"], r))


def test_enumerated_game_through_pointnet_at_16_regions_is_the_exact_index():
    data, lbl, rid, args = _game("pointnet", 1024, 16)
    model, _ = probes.coalition_model("pointnet", DEV)
    g = kernelshap.game(model, data, lbl, rid, args, samples="all", pairs=True)
    without = kernelshap.game(model, data, lbl, rid, args, samples="all")
    assert "interaction" not in without and np.array_equal(without["phi"], g["phi"])
    v = exact.value_table(model, data, lbl, rid, args)
    want = _exact_sii(v, 16)
    vh = v.cpu().numpy()
    keep = _u64(g["keep"]).reshape(-1, 1)
    bound = ref.bound(keep, g["v"].cpu().numpy(), g["v_empty"], 16, g["weights"].cpu().numpy())
    vmax = float(np.abs(vh).max())
    err = float(np.abs(g["interaction"] - want).max())
    print("PointNet R=16 enumerated: max |pairs - exact| = %.3g, bound %.3g + %.3g; rms of the exact index %.3g"
          % (err, bound, 9 * 2.0 ** -24 * vmax, float(np.sqrt((want[np.triu_indices(16, 1)] ** 2).mean()))))
    assert g["interaction"].shape == (16, 16) and err <= 9 * 2.0 ** -24 * vmax + bound


def test_sampled_game_through_pointnet_at_32_regions():
    data, lbl, rid, args = _game("pointnet", 1024, 32)
    model, _ = probes.coalition_model("pointnet", DEV)
    np.random.seed(41)
    g = kernelshap.game(model, data, lbl, rid, args, samples=2000, counts=(), pairs=True)
    _sampled(g, 32, "PointNet R=32")
    np.random.seed(41)
    both = kernelshap.play(kernelshap, model, data, None, rid, args, 2000, counts=(), classes=[int(lbl), 0], pairs=True)
    assert both["interaction"].shape == (2, 32, 32) and np.array_equal(both["interaction"][0], g["interaction"])


@pytest.mark.parametrize("n,r", [(256, 65), (128, 128)])
def test_sampled_wide_game_through_pointnet(n, r):
    data, lbl, rid, args = _game("pointnet", n, r)
    model, _ = probes.coalition_model("pointnet", DEV)
    np.random.seed(43)
    _sampled(wide_kernelshap.game(model, data, lbl, rid, args, samples=600, counts=(), pairs=True), r, "PointNet wide R=%d" % r)


def test_sampled_wide_game_through_pointnet2_on_compact_coalitions():
    data, lbl, rid, args = _game("pointnet2", 128, 65)
    model, _ = probes.coalition_model("pointnet2", DEV)
    np.random.seed(47)
    _sampled(wide_kernelshap.game(model, data, lbl, rid, args, samples=200, counts=(), coalitions="compact", pairs=True), 65,
             "PointNet++ R=65 compact")


# ---- drivers ----

def _run(script, cwd, extra):
    env = dict(os.environ, PYTHONPATH=REPO)
    cmd = [sys.executable, os.path.join(REPO, script), "--model", "pointnet", "--dataset", "modelnet10", "--synthetic", "--num_clouds", "2"] + extra
    r = subprocess.run(cmd, cwd=str(cwd), env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


def _same_files(a, b, skip):
    """Every file of folder ``b`` (the run without --pairs) is in ``a`` with the same bytes; ``a`` has ``skip`` beside them."""
    names = sorted(os.listdir(b))
    assert sorted(os.listdir(a)) == sorted(names + list(skip)), (sorted(os.listdir(a)), names)
    return [n for n in names if (a / n).read_bytes() != (b / n).read_bytes()]


def test_final_kernel_shapley_with_pairs(tmp_path):
    """One child with --compare_exact --pairs, one with --compare_exact alone: the flag adds region_interaction.npy and the
    "pairs" object of sampling_error.json, and changes no other byte."""
    flags = ["--num_regions", "8", "--samples", "512", "--compare_exact"]
    (tmp_path / "with").mkdir()
    (tmp_path / "without").mkdir()
    _run("final_kernel_shapley.py", tmp_path / "with", flags + ["--pairs"])
    _run("final_kernel_shapley.py", tmp_path / "without", flags)
    folder = "exp_MODEL_pointnet_DATA_modelnet10_POINTNUM_1024_REGIONNUM_8_shapley_test"
    for cloud in ("synthetic_00", "synthetic_01"):
        a, b = (tmp_path / w / "checkpoints" / folder / cloud / "kernelshap" for w in ("with", "without"))
        assert _same_files(a, b, ["region_interaction.npy"]) == ["sampling_error.json"]
        ja, jb = json.load(open(a / "sampling_error.json")), json.load(open(b / "sampling_error.json"))
        pairs_error = ja.pop("pairs")
        assert ja == jb and "pairs" not in jb
        assert set(pairs_error) == {"max_abs_error", "rms_error"} and all(np.isfinite(x) and x >= 0 for x in pairs_error.values())
        assert pairs_error["rms_error"] <= pairs_error["max_abs_error"]
        got = np.load(a / "region_interaction.npy")
        assert got.shape == (8, 8) and got.dtype == np.float64
        keep = torch.from_numpy(np.load(a / "coalitions.npy").view(np.int64)).to(DEV)
        v = torch.from_numpy(np.load(a / "rewards.npy")).to(DEV)
        assert np.array_equal(got, kernelshap.pairs(keep, v, ja["v_empty"], ja["v_full"], 8))


def test_final_wide_kernel_shapley_with_pairs(tmp_path, monkeypatch):
    """One child with --pairs, one without: the flag adds region_interaction.npy and draw.json's "pairs", and changes no other
    byte.  The file is ``pairs`` of the stored rows and rewards, the two end rewards evaluated again in this process."""
    from interpret_quality_amd import shapley_stage, wide_kernel_stage, wide_stage
    from interpret_quality_amd.final_util import get_folder_name_list, load_model
    flags = ["--num_regions", "65", "--samples", "400"]
    (tmp_path / "with").mkdir()
    (tmp_path / "without").mkdir()
    _run("final_wide_kernel_shapley.py", tmp_path / "with", flags + ["--pairs"])
    _run("final_wide_kernel_shapley.py", tmp_path / "without", flags)
    folder = "exp_MODEL_pointnet_DATA_modelnet10_POINTNUM_1024_REGIONNUM_65_shapley_test"
    for cloud in ("synthetic_00", "synthetic_01"):
        a, b = (tmp_path / w / "checkpoints" / folder / cloud / "kernelshap" for w in ("with", "without"))
        assert _same_files(a, b, ["region_interaction.npy"]) == ["draw.json"]
        ja, jb = json.load(open(a / "draw.json")), json.load(open(b / "draw.json"))
        assert ja.pop("pairs") is True and ja == jb
    monkeypatch.chdir(tmp_path / "with")
    args = wide_kernel_stage.make_args(["--model", "pointnet", "--dataset", "modelnet10", "--synthetic", "--num_clouds", "2"] + flags)
    shapley_stage.finish_args(args)
    model = load_model(args)
    seen = 0
    with torch.no_grad():
        for i, name, result_path, data, lbl, fps_index in shapley_stage.selected_clouds(args, get_folder_name_list(args), None):
            rid = wide_stage.cal_region_id(data, fps_index, result_path, save=False)
            keep = torch.from_numpy(np.load(result_path + "kernelshap/coalitions.npy").view(np.int64)).to(DEV)
            stored = torch.from_numpy(np.load(result_path + "kernelshap/rewards.npy")).to(DEV)
            v, v_full, v_empty = wide_kernelshap.rewards(model, data, lbl, rid, args, keep, args.coalitions)
            assert torch.equal(v, stored)
            got = np.load(result_path + "kernelshap/region_interaction.npy")
            assert got.shape == (65, 65) and got.dtype == np.float64
            assert np.array_equal(got, wide_kernelshap.pairs(keep, stored, v_empty, v_full, 65))
            seen += 1
    assert seen == 2
