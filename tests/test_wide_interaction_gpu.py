"""GPU: multi-order interactions of wide games - (pair, context) coalitions over more than 64 regions, up to one region per point
(iq_context_keep_masks_wide, interpret_quality_amd/wide.py, final_wide_interaction.py).

Bars (none is new):
  * masks = the host twin, wide = narrow at R <= 64, fused = dense on materialised clouds, launch independence, the m = 0
    interaction from hand-built rows: bitwise;
  * logits against oracle.ref_cpu.compute_order_interaction_logits: 1e-4 element-wise with a floor
    (conftest.assert_close_elementwise), PointNet (fused) and PointNet++ (dense route);
  * interactions against oracle.ref_cpu.compute_order_interaction: |dI| <= 1e-4 max|v|.
"""
import argparse
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import probes
from conftest import REPO, assert_close_elementwise
from interpret_quality_amd import _lib, final_common, hip_ops, interaction, synth, wide
from oracle import ref_cpu

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _args(family="pointnet", num_regions=128):
    return argparse.Namespace(model=family, softmax_type="modified", num_points=1024, num_regions=num_regions, verbose=False,
                              interaction_batch_size=25)


def _cloud(i, n=1024):
    pts, y = synth.make_cloud(i, n)
    return torch.from_numpy(pts)[None], torch.tensor([y])


_RID = {}


def _regions(i, r):
    """Cloud i and the oracle's region ids for the oracle's r FPS centres ((N,) int64); r = N: a seeded one-point-per-region map."""
    if (i, r) not in _RID:
        data, lbl = _cloud(i)
        if r == data.shape[1]:
            rid = np.random.default_rng(i).permutation(r)
        else:
            rid = np.asarray(ref_cpu.cal_region_id(data, ref_cpu.farthest_point_sample(data, r)[0].numpy())).astype(np.int64)
        _RID[(i, r)] = (data, lbl, rid)
    return _RID[(i, r)]


def _pairs_contexts(rng, r, p, c, m):
    """p random pairs (the first one straddles a word boundary when there is one) and c contexts of m regions for each."""
    pairs = np.stack([rng.choice(r, size=2, replace=False) for _ in range(p)]).astype(np.int64)
    if r > 64:
        pairs[0] = (64, 63)
    ctx = np.stack([np.stack([rng.permutation(np.setdiff1d(np.arange(r), pr))[:m] for _ in range(c)]).reshape(c, m) for pr in pairs])
    return pairs, ctx.astype(np.int64)


def _device_masks(pairs, ctx, r):
    keep = hip_ops.context_keep_masks_wide(hip_ops.as_i32(pairs, DEV), hip_ops.as_i32(ctx, DEV), r)
    assert keep.dtype == torch.int64 and tuple(keep.shape) == (4 * ctx.shape[0] * ctx.shape[1], (r + 63) // 64)
    return keep


# ---- 1. masks ----

@pytest.mark.parametrize("r", [65, 128, 200, 1024])
def test_device_masks_equal_the_host_twin(r):
    rng = np.random.default_rng(r)
    for m in (0, 1, 63, 64, 65, r - 2):
        if m > r - 2:
            continue
        pairs, ctx = _pairs_contexts(rng, r, 3, 5, m)            # 15 contexts: the last workgroup of four is not full
        got = _device_masks(pairs, ctx, r).cpu().numpy().view(np.uint64)
        assert np.array_equal(got, wide.context_keep_masks(pairs, ctx, r)), (r, m)
    # the context of every other region: the four rows hold R, R-1, R-1 and R-2 regions, nothing at or above R
    full = _device_masks(pairs, ctx, r).cpu().numpy().view(np.uint64)
    bits = ((full[:, :, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).reshape(full.shape[0], -1)
    assert np.array_equal(bits.sum(axis=1).reshape(-1, 4), np.tile([r, r - 1, r - 1, r - 2], (15, 1))) and not bits[:, r:].any()


@pytest.mark.parametrize("r", [65, 1024])
def test_invalid_pair_and_context_entries_are_ignored(r):
    rng = np.random.default_rng(r + 7)
    pairs, ctx = _pairs_contexts(rng, r, 3, 3, 70 if r > 72 else 40)
    ctx[0, 0, 3], ctx[1, 2, 0], ctx[2, 1, -1], ctx[2, 2, 5] = r, -1, 2 ** 31 - 1, r + 63
    pairs[1, 0], pairs[2, 1] = r, -5
    got = _device_masks(pairs, ctx, r).cpu().numpy().view(np.uint64)
    assert np.array_equal(got, wide.context_keep_masks(pairs, ctx, r))
    bits = ((got[:, :, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).reshape(got.shape[0], -1)
    assert not bits[:, r:].any()
    assert np.array_equal(got[12], got[14]) and np.array_equal(got[13], got[15])      # pair 1 lost its region i


@pytest.mark.parametrize("r", [32, 64])
def test_device_masks_equal_the_narrow_kernel_up_to_64_regions(r):
    rng = np.random.default_rng(r)
    for m in (0, 1, (r - 2) // 2, r - 2):
        pairs, ctx = _pairs_contexts(rng, r, 7, 9, m)
        narrow = hip_ops.context_keep_masks(hip_ops.as_i32(pairs, DEV), hip_ops.as_i32(ctx, DEV))
        assert torch.equal(_device_masks(pairs, ctx, r)[:, 0], narrow), (r, m)


def test_wrapper_refuses_bad_arguments_and_takes_empty_lists():
    pairs = torch.zeros((2, 2), dtype=torch.int32, device=DEV)
    ctx = torch.zeros((2, 3, 5), dtype=torch.int32, device=DEV)
    for bad_pairs, bad_ctx, r in ((pairs, ctx, 1025), (pairs, ctx, 0), (pairs, ctx, 4), (pairs, ctx[:1].contiguous(), 128),
                                  (pairs.long(), ctx, 128), (pairs, ctx.long(), 128), (pairs.cpu(), ctx, 128), (pairs, ctx[:, :, 0], 128)):
        with pytest.raises(_lib.IqError):
            hip_ops.context_keep_masks_wide(bad_pairs, bad_ctx, r)
    assert tuple(hip_ops.context_keep_masks_wide(pairs[:0].contiguous(), ctx[:0].contiguous(), 128).shape) == (0, 2)
    assert tuple(hip_ops.context_keep_masks_wide(pairs, ctx[:, :0].contiguous(), 128).shape) == (0, 2)
    model, _ = probes.coalition_model("pointnet", DEV)
    data, _, rid = _regions(0, 128)
    out = wide.interaction_logits(model, data.to(DEV), rid, np.zeros((0, 2), dtype=np.int64), np.zeros((0, 4, 3), dtype=np.int64), _args())
    assert tuple(out.shape) == (0, 16, 10)
    with pytest.raises(_lib.IqError):       # the API names a bad index instead of ignoring it
        wide.interaction_logits(model, data.to(DEV), rid, np.array([[0, 1]]), np.array([[[5, 128]]]), _args())


# ---- 2. logits ----

def test_wide_equals_the_narrow_stage_bitwise_at_64_regions(capsys):
    r = 64
    model, _ = probes.coalition_model("pointnet", DEV)
    data, _, rid = _regions(1, r)
    rng = np.random.default_rng(64)
    for m in (0, 5, 31, 62):
        pairs, ctx = _pairs_contexts(rng, r, 6, 1 if m in (0, 62) else 7, m)
        got = wide.interaction_logits(model, data.to(DEV), rid, pairs, ctx, _args("pointnet", r))
        narrow = interaction.compute_order_interaction_logits(model, data.to(DEV), rid, pairs, ctx, _args("pointnet", r))
        assert got.dtype == torch.float32 and tuple(got.shape) == (6, 4 * ctx.shape[1], 10) and torch.equal(got, narrow), m
    capsys.readouterr()


@pytest.mark.parametrize("r", [128, 1024])
def test_fused_logits_equal_the_dense_forward_on_materialised_clouds_bitwise(r):
    model, _ = probes.coalition_model("pointnet", DEV)
    data, _, rid = _regions(2, r)
    pairs, ctx = _pairs_contexts(np.random.default_rng(r), r, 5, 9, (r - 2) // 2)
    d = data.to(DEV)
    got = wide.interaction_logits(model, d, rid, pairs, ctx, _args("pointnet", r))
    keep = _device_masks(pairs, ctx, r)
    masked = hip_ops.mask_coalitions_wide(d[0].contiguous(), hip_ops.as_i32(rid, DEV), keep, d.mean(dim=1).reshape(3).contiguous(), r,
                                          channel_first=True)
    dense = model(masked)[0]
    assert tuple(got.shape) == (5, 36, 10) and torch.isfinite(got).all()
    assert torch.equal(got.reshape(-1, 10), dense)


_ORACLE = {}


def _oracle_case():
    """PointNet, R = 128, 3 pairs x 4 contexts x ratios {0, 0.5, 1}: ours and the oracle's logits, computed once."""
    if not _ORACLE:
        r = 128
        model, sd = probes.coalition_model("pointnet", DEV)
        data, lbl, rid = _regions(0, r)
        rng = np.random.default_rng(128)
        cases = []
        for ratio in (0.0, 0.5, 1.0):
            m = int((r - 2) * ratio)
            pairs, ctx = _pairs_contexts(rng, r, 3, 4, m)
            got = wide.interaction_logits(model, data.to(DEV), rid, pairs, ctx, _args("pointnet", r))
            want = ref_cpu.compute_order_interaction_logits(ref_cpu.PointNetOracle(sd), data, rid, pairs, ctx, 4)
            cases.append((m, pairs, ctx, got, want))
        _ORACLE.update(data=data, lbl=lbl, rid=rid, cases=cases)
    return _ORACLE


def test_pointnet_logits_match_the_oracle_at_128_regions():
    for m, _, _, got, want in _oracle_case()["cases"]:
        assert tuple(got.shape) == tuple(want.shape) == (3, 16, 10)
        print("pointnet R=128 m=%d vs oracle: max |d| / max |logit| = %.3g" % (m, probes.rel_max_err(got.cpu().numpy(), want.numpy())))
        assert_close_elementwise(got.cpu().numpy(), want.numpy(), rtol=1e-4)


def test_interactions_match_the_oracle_at_128_regions():
    o = _oracle_case()
    args = _args("pointnet", 128)
    for m, _, _, got, want in o["cases"]:
        mine = wide.interactions(got, o["lbl"].to(DEV), args)
        ref = ref_cpu.compute_order_interaction(want, o["lbl"])
        vmax = float(ref_cpu.get_reward(want.reshape(-1, 10), o["lbl"]).abs().max())
        print("pointnet R=128 m=%d: max |dI| / max |v| = %.3g" % (m, float(np.abs(mine - ref).max()) / vmax))
        assert mine.shape == ref.shape == (3, 4) and mine.dtype == np.float64
        assert np.abs(mine - ref).max() <= 1e-4 * vmax


@pytest.mark.parametrize("ratio", [0.0, 0.5, 1.0])
def test_pointnet2_runs_the_dense_route_and_matches_the_oracle(ratio):
    r = 128
    model, sd = probes.coalition_model("pointnet2", DEV)
    data, lbl, rid = _regions(0, r)
    args = _args("pointnet2", r)
    pairs, ctx = _pairs_contexts(np.random.default_rng(2), r, 1, 4, int((r - 2) * ratio))
    got = wide.interaction_logits(model, data.to(DEV), rid, pairs, ctx, args)
    want = ref_cpu.compute_order_interaction_logits(ref_cpu.PointNet2Oracle(sd), data, rid, pairs, ctx, 4, is_pointnet=False)
    print("pointnet2 R=128 ratio %.1f vs oracle: max |d| / max |logit| = %.3g" % (ratio, probes.rel_max_err(got.cpu().numpy(), want.numpy())))
    assert tuple(got.shape) == (1, 16, 10)
    assert_close_elementwise(got.cpu().numpy(), want.numpy(), rtol=1e-4)
    mine, ref = wide.interactions(got, lbl.to(DEV), args), ref_cpu.compute_order_interaction(want, lbl)
    assert np.abs(mine - ref).max() <= 1e-4 * float(ref_cpu.get_reward(want.reshape(-1, 10), lbl).abs().max())


def test_the_empty_context_interaction_equals_the_four_hand_built_coalitions():
    r = 128
    model, _ = probes.coalition_model("pointnet", DEV)
    data, lbl, rid = _regions(0, r)
    args = _args("pointnet", r)
    pairs = np.array([[64, 63], [0, 127], [100, 3]])
    logits = wide.interaction_logits(model, data.to(DEV), rid, pairs, np.zeros((3, 1, 0), dtype=np.int64), args)
    got = wide.interactions(logits, lbl.to(DEV), args)
    assert got.shape == (3, 1)
    for p, (i, j) in enumerate(pairs):
        rows = np.zeros((4, 2), dtype=np.uint64)
        for q, members in enumerate(((i, j), (i,), (j,), ())):
            for x in members:
                rows[q, x >> 6] |= np.uint64(1) << np.uint64(x & 63)
        v = final_common.get_reward(wide.coalition_logits(model, data.to(DEV), rid, rows, args), lbl.to(DEV), args).cpu().numpy()
        assert v.dtype == np.float32
        assert got[p, 0] == np.float64(((v[0] + v[3]) - v[1]) - v[2])


def test_logits_do_not_depend_on_the_launch():
    r = 128
    model, _ = probes.coalition_model("pointnet", DEV)
    data, _, rid = _regions(3, r)
    pairs, ctx = _pairs_contexts(np.random.default_rng(9), r, 10, 25, 63)
    args = _args("pointnet", r)
    big = wide.interaction_logits(model, data.to(DEV), rid, pairs, ctx, args)               # 1000 coalitions, one launch
    part = wide.interaction_logits(model, data.to(DEV), rid, pairs[4:5], ctx[4:5, 7:8], args)
    assert torch.equal(part[0], big[4, 28:32])
    cap = type(model).max_wide_per_call
    try:
        type(model).max_wide_per_call = 300                                               # four launches, the last one short
        assert torch.equal(wide.interaction_logits(model, data.to(DEV), rid, pairs, ctx, args), big)
    finally:
        type(model).max_wide_per_call = cap


# ---- 3. the drivers ----

def _env():
    env = dict(os.environ, PYTHONPATH=REPO)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "IQ_FORCE_DIST", "IQ_REHEARSAL"):
        env.pop(k, None)
    return env


COMMON = ["--model", "pointnet", "--dataset", "modelnet10", "--synthetic", "--num_clouds", "1"]


def test_final_wide_interaction_script_end_to_end(tmp_path, monkeypatch, capsys):
    from interpret_quality_amd import wide_interaction_stage, wide_stage
    monkeypatch.chdir(tmp_path)
    wide_stage.main(COMMON + ["--num_samples_save", "4", "--num_regions", "128"])           # region_id.npy of the 128-region game
    root = tmp_path / "checkpoints" / "exp_MODEL_pointnet_DATA_modelnet10_POINTNUM_1024_REGIONNUM_128_shapley_test" / "synthetic_00"
    region_id = np.load(root / "region_id.npy")
    np.save(tmp_path / "pose.npy", np.array([0.4, -0.3, 0.2]))
    import gc
    gc.collect()
    torch.cuda.empty_cache()            # the child shares this GPU: hand back what the caching allocator holds
    cmd = [sys.executable, os.path.join(REPO, "final_wide_interaction.py")] + COMMON + [
        "--num_regions", "128", "--num_pairs_random", "3", "--num_save_context_max", "4", "--mode", "rotate",
        "--transform_params", str(tmp_path / "pose.npy")]
    run = subprocess.run(cmd, cwd=str(tmp_path), env=_env(), capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-3000:]
    inter = root / "interaction_seed1"
    pairs = np.load(inter / "region_pair_list.npy")
    assert pairs.shape == (3, 2) and pairs.dtype == np.int64 and np.all(pairs[:, 0] < pairs[:, 1]) and pairs.max() < 128
    # the stream of final_gen_pair.py --seed 1: pairs first, then the contexts ratio by ratio
    from interpret_quality_amd.final_util import set_random
    set_random(1)
    want_pairs = wide.gen_pair_random(argparse.Namespace(num_regions=128, num_pairs_random=3))
    want_ctx = wide.gen_context(want_pairs, 128, interaction.DEFAULT_RATIOS, 4)
    assert np.array_equal(pairs, want_pairs)
    lab = np.load(inter / "rotate_adv" / "pred_labels.npy")
    assert lab.shape == (2,) and lab[0] == 0
    assert np.array_equal(np.load(inter / "rotate_adv" / "transform_params.npy"), np.array([0.4, -0.3, 0.2]))
    for ratio, want in zip(interaction.DEFAULT_RATIOS, want_ctx):
        tag = "ratio%d" % int(ratio * 100)
        m = int(126 * ratio)
        ctx = np.load(inter / (tag + "_context_list.npy"))
        assert ctx.dtype == np.int16 and ctx.shape == (3, 1 if m in (0, 126) else 4, m) and np.array_equal(ctx, want)
        for sub in ("normal", "rotate_adv"):
            lg = torch.load(inter / sub / (tag + "_all_logits.pt"))
            it = np.load(inter / sub / (tag + "_pred_interaction.npy"))
            assert lg.dtype == torch.float32 and tuple(lg.shape) == (3, 4 * ctx.shape[1], 10)
            assert it.dtype == np.float64 and it.shape == (3, ctx.shape[1])
    # the API on the same cloud, regions, pairs and contexts: the same bits, at both poses
    model, _ = probes.coalition_model("pointnet", DEV)
    data, lbl = _cloud(0)
    args = _args("pointnet", 128)
    ctx50 = np.load(inter / "ratio50_context_list.npy")
    saved = torch.load(inter / "normal" / "ratio50_all_logits.pt", map_location=DEV)
    assert torch.equal(saved, wide.interaction_logits(model, data.to(DEV), region_id, pairs, ctx50, args))
    assert np.array_equal(np.load(inter / "normal" / "ratio50_pred_interaction.npy"), wide.interactions(saved, lbl.to(DEV), args))
    from interpret_quality_amd.pose_sweep import rotate_xyz
    turned = rotate_xyz(data.to(DEV), torch.tensor([0.4, -0.3, 0.2], device=DEV))
    saved_adv = torch.load(inter / "rotate_adv" / "ratio50_all_logits.pt", map_location=DEV)
    assert torch.equal(saved_adv, wide.interaction_logits(model, turned, region_id, pairs, ctx50, args))
    pred = torch.tensor([int(lab[1])], device=DEV)
    assert np.array_equal(np.load(inter / "rotate_adv" / "ratio50_pred_interaction.npy"), wide.interactions(saved_adv, pred, args))
    # outside 65 .. 1024 regions the driver refuses, and so it does without the stage-1 folder of its region count
    with pytest.raises(SystemExit):
        wide_interaction_stage.main(COMMON + ["--num_regions", "64"])
    with pytest.raises(SystemExit):
        wide_interaction_stage.main(COMMON + ["--num_regions", "200"])
    capsys.readouterr()


def test_final_point_binary_interaction_logits_is_unchanged_at_32_regions(tmp_path, monkeypatch, capsys):
    """The narrow stage on hand-made stage-1 artefacts: it writes what interaction.compute_order_interaction_logits returns, and at
    32 regions those are the bits of the wide route too."""
    from interpret_quality_amd import shapley_stage
    monkeypatch.chdir(tmp_path)
    shapley_stage.main(COMMON + ["--num_samples_save", "4"])
    root = tmp_path / "checkpoints" / "exp_MODEL_pointnet_DATA_modelnet10_POINTNUM_1024_REGIONNUM_32_shapley_test" / "synthetic_00"
    inter = root / "interaction_seed1"
    os.makedirs(inter / "normal")
    os.makedirs(inter / "rotate_adv")
    np.random.seed(5)
    pairs = np.array([[1, 5], [7, 30], [0, 31]])
    np.save(inter / "region_pair_list.npy", pairs)
    contexts = wide.gen_context(pairs, 32, interaction.DEFAULT_RATIOS, 3)
    for ratio, ctx in zip(interaction.DEFAULT_RATIOS, contexts):
        np.save(inter / ("ratio%d_context_list.npy" % int(ratio * 100)), ctx)
    np.save(inter / "rotate_adv" / "transform_params.npy", np.array([0.4, -0.3, 0.2]))
    interaction.main_logits(COMMON)
    model, _ = probes.coalition_model("pointnet", DEV)
    data, _ = _cloud(0)
    region_id = np.load(root / "region_id.npy")
    args = _args("pointnet", 32)
    for ratio, ctx in zip(interaction.DEFAULT_RATIOS, contexts):
        saved = torch.load(inter / "normal" / ("ratio%d_all_logits.pt" % int(ratio * 100)), map_location=DEV)
        assert tuple(saved.shape) == (3, 4 * ctx.shape[1], 10)
        assert torch.equal(saved, interaction.compute_order_interaction_logits(model, data.to(DEV), region_id, pairs, ctx, args))
        assert torch.equal(saved, wide.interaction_logits(model, data.to(DEV), region_id, pairs, ctx, args))
    assert len([f for f in os.listdir(inter / "rotate_adv") if f.endswith("_all_logits.pt")]) == len(interaction.DEFAULT_RATIOS)
    capsys.readouterr()
