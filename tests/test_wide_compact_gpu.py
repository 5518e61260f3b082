"""GPU: the compact coalition paths of PointNet++, DGCNN, GCNN and PointConv for wide games (iq_*_coalitions_wide,
``coalition_logits_wide``, ``wide.*(coalitions="compact")``).

Only the few small kernels that turn a mask into a coalition's kept points have a wide form; everything behind them works on points.
So the bars are those of the narrow compact paths, none is new:
  * wide entry = narrow entry on the same mask (R <= 64) and on the same kept points (R > 64), launch independence, cached tables,
    ``coalitions="dense"`` = the dense forward: bitwise;
  * compact against the family's dense forward on the clouds iq_mask_coalitions_wide writes: 2e-5 of max |logit|
    (tests/test_pointconv_gpu.py); DGCNN and GCNN: the bars of tests/test_dgcnn_gpu.py - 1e-5 on 1024-point clouds
    (test_compact_coalitions_equal_the_dense_forward_on_masked_clouds), 2e-5 on small ones
    (test_coalitions_on_clouds_of_barely_more_than_k_points);
  * against the CPU oracle: probes.COALITION_RTOL (pointnet2, gcnn, pointconv);
  * efficiency of a permutation row: R float32 roundings of at most 2 max|v| 2^-24 each; Shapley values compact against dense:
    1e-4 norm-wise.
"""
import argparse
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import probes
from conftest import REPO
from interpret_quality_amd import _lib, final_common, hip_ops, synth, wide

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FAMILIES = ["pointnet2", "dgcnn", "gcnn", "pointconv"]
SMALL_N = {"pointnet2": 128, "pointconv": 64, "dgcnn": 96, "gcnn": 96}    # the smallest cloud a family's compact path takes


def _args(family, num_regions, num_points=1024):
    return argparse.Namespace(model=family, softmax_type="modified", num_points=num_points, num_regions=num_regions, verbose=False)


def _clouds(n, nc=1, first=0):
    pts = np.stack([synth.make_cloud(first + i, n)[0] for i in range(nc)])
    clouds = torch.from_numpy(pts).to(DEV).contiguous()
    return clouds, clouds.mean(dim=1).contiguous()


_RID64 = {}


def _fps_rid64(clouds):
    """A 64-region game from FPS on the device: (nc, N) int32 device tensor (computed once per cloud set)."""
    key = (clouds.shape, float(clouds[0, 0, 0]))
    if key not in _RID64:
        rows = []
        for c in range(clouds.shape[0]):
            fps = hip_ops.fps(clouds[c:c + 1], 64)[0].contiguous()
            rows.append(hip_ops.region_assign_wide(clouds[c].contiguous(), fps))
        _RID64[key] = torch.stack(rows).contiguous()
    return _RID64[key]


def _narrow_masks(rng, count, r):
    """``count`` random masks over r regions of all sizes, plus the empty, the full and a one-bit mask: Python ints."""
    full = (1 << r) - 1
    member = rng.random((count, r)) < rng.random((count, 1))
    masks = [int(sum(1 << int(j) for j in np.flatnonzero(row))) for row in member]
    return masks + [0, full, 1 << (r // 2)]


def _wide_rows(masks, words):
    """Narrow masks -> (B, words) uint64 rows with every word equal to the mask."""
    return np.repeat(np.array(masks, dtype=np.uint64)[:, None], words, axis=1)


# ---- 1. wide entry = narrow entry at R <= 64 ----

@pytest.mark.parametrize("family,n", [(f, SMALL_N[f]) for f in FAMILIES] + [(f, 1024) for f in FAMILIES])
def test_wide_entry_equals_narrow_entry_bitwise_up_to_64_regions(family, n):
    model, _ = probes.coalition_model(family, DEV)
    clouds, centers = _clouds(n, nc=2)
    for r in (32, 64):
        rng = np.random.default_rng(1000 * r + n)
        rid = torch.from_numpy(rng.integers(0, r, size=(2, n)).astype(np.int32)).to(DEV)
        masks = _narrow_masks(rng, 57, r)
        cloud_of = torch.from_numpy(rng.integers(0, 2, size=len(masks)).astype(np.int32)).to(DEV)
        keep = hip_ops.masks_to_tensor(masks, DEV)
        narrow = model.coalition_logits(clouds, centers, rid, keep, cloud_of, num_regions=r).clone()
        got = model.coalition_logits_wide(clouds, centers, rid, keep.reshape(-1, 1).contiguous(), cloud_of, num_regions=r)
        assert got.shape == narrow.shape and torch.isfinite(got).all()
        assert torch.equal(got, narrow), (family, n, r)


# ---- 2. above 64 regions: the narrow path's bits on the same kept points ----

def _split_case(family, n, parts):
    """rid0: 64 FPS regions; every region split ``parts`` ways by point index -> R = 64 * parts; a wide row whose words all equal m
    keeps exactly the points narrow mask m keeps."""
    clouds, centers = _clouds(n, first=3)
    rid0 = _fps_rid64(clouds)
    idx = torch.arange(n, device=DEV, dtype=torch.int32)
    rid = (rid0 + 64 * (idx % parts)[None]).contiguous()
    return clouds, centers, rid0, rid


@pytest.mark.parametrize("parts", [2, 3])
@pytest.mark.parametrize("family,n", [(f, 1024) for f in FAMILIES] + [("pointnet2", 128), ("pointconv", 128)])
def test_words_one_and_up_select_the_same_points_as_the_narrow_mask_bitwise(family, n, parts):
    model, _ = probes.coalition_model(family, DEV)
    clouds, centers, rid0, rid = _split_case(family, n, parts)
    masks = _narrow_masks(np.random.default_rng(7 * n + parts), 40, 64)
    narrow = model.coalition_logits(clouds, centers, rid0, hip_ops.masks_to_tensor(masks, DEV), None, num_regions=64).clone()
    rows = hip_ops.wide_masks_to_tensor(_wide_rows(masks, parts), DEV)
    got = model.coalition_logits_wide(clouds, centers, rid, rows, None, num_regions=64 * parts)
    assert torch.equal(got, narrow), (family, n, parts)
    # a row that differs from the narrow mask in ONE word keeps other points: the words are really read
    if parts == 3:
        other = _wide_rows(masks[:8], parts)
        other[:, 2] = ~other[:, 2]
        changed = model.coalition_logits_wide(clouds, centers, rid, hip_ops.wide_masks_to_tensor(other, DEV), None, num_regions=192)
        assert not torch.equal(changed, narrow[:8])


# ---- 3. shapes of the row ----

def _row_case(n, r):
    """The coalitions of a row shape: empty, full, only region 64 (R <= 64: region R / 2), only region R-1, a random one with every
    bit at and above R set as well, and the same one with those bits cleared.  -> (rows (6,W) uint64, the rows without such bits)."""
    w = (r + 63) // 64
    rng = np.random.default_rng(r * 31 + n)
    one = 64 if r > 64 else r // 2
    rows = np.zeros((6, w), dtype=np.uint64)
    rows[1, :] = ~np.uint64(0)
    rows[2, one >> 6] = np.uint64(1) << np.uint64(one & 63)
    rows[3, (r - 1) >> 6] = np.uint64(1) << np.uint64((r - 1) & 63)
    rows[4] = rng.integers(0, 2 ** 64, size=w, dtype=np.uint64)
    rows[5] = rows[4]
    clean = rows.copy()
    if r & 63:
        low = np.uint64((1 << (r & 63)) - 1)
        clean[:, w - 1] &= low
        rows[5, w - 1] = clean[4, w - 1]
        rows[4, w - 1] |= ~low
    return rows, clean


def _row_shapes(family):
    """(N, R, with the oracle): R = 65 and R = 128 on 128 points, one region per point at the family's smallest cloud and at 1024."""
    return [(128, 65, False), (128, 128, True), (SMALL_N[family], SMALL_N[family], False), (1024, 1024, False)]


@pytest.mark.parametrize("family", FAMILIES)
def test_row_shapes_against_the_dense_forward_and_the_oracle(family):
    model, sd = probes.coalition_model(family, DEV)
    for n, r, with_oracle in _row_shapes(family):
        clouds, centers = _clouds(n, first=5)
        rng = np.random.default_rng(n + r)
        if r == n:
            rid_h = rng.permutation(n)                             # one region per point
        else:
            rid_h = rng.integers(0, r, size=n)
            rid_h[:r] = np.arange(r)                               # no region is empty
        rid = hip_ops.as_i32(rid_h[None], DEV)
        rows, clean = _row_case(n, r)
        kw = hip_ops.wide_masks_to_tensor(rows, DEV)
        got = model.coalition_logits_wide(clouds, centers, rid, kw, None, num_regions=r).clone()
        assert got.shape == (6, 10) and torch.isfinite(got).all()
        # bits at or above R change nothing
        assert torch.equal(got[4], got[5]), (family, n, r)
        again = model.coalition_logits_wide(clouds, centers, rid, hip_ops.wide_masks_to_tensor(clean, DEV), None, num_regions=r)
        assert torch.equal(again, got)
        masked = hip_ops.mask_coalitions_wide(clouds[0].contiguous(), rid[0].contiguous(), kw, centers[0].contiguous(), r)
        dense = model.forward_points(masked)
        err = probes.rel_max_err(got.cpu().numpy(), dense.cpu().numpy())
        bar = 2e-5 if family in ("pointnet2", "pointconv") or n < 1024 else 1e-5     # module docstring
        print("%s N=%d R=%d compact vs dense: %.3g (bar %.3g)" % (family, n, r, err, bar))
        assert err < bar, (family, n, r, err)
        if with_oracle and family != "dgcnn":
            want = probes.oracle_logits(family, sd, masked.cpu())
            oerr = probes.rel_max_err(got.cpu().numpy(), want)
            print("%s N=%d R=%d compact vs oracle: %.3g" % (family, n, r, oerr))
            assert oerr <= probes.COALITION_RTOL, (family, n, r, oerr)


# ---- 4. both DGCNN / GCNN layouts ----

@pytest.mark.parametrize("family", ["dgcnn", "gcnn"])
@pytest.mark.parametrize("b", [3, 40])
def test_graph_families_with_and_without_the_list_walk(family, b):
    """B = 3 coalitions of one cloud: nclouds * 8 > B, the layer-1 graph comes from knn_kernel; B = 40: from dg_walk_kernel."""
    model, _ = probes.coalition_model(family, DEV)
    clouds, centers, rid0, rid = _split_case(family, 1024, 2)
    masks = _narrow_masks(np.random.default_rng(b), b - 3, 64)
    narrow = model.coalition_logits(clouds, centers, rid0, hip_ops.masks_to_tensor(masks, DEV), None, num_regions=64).clone()
    got = model.coalition_logits_wide(clouds, centers, rid, hip_ops.wide_masks_to_tensor(_wide_rows(masks, 2), DEV), None,
                                      num_regions=128)
    assert got.shape == (b, 10) and torch.equal(got, narrow)


# ---- 5. launch independence ----

@pytest.mark.parametrize("family", FAMILIES)
def test_logits_do_not_depend_on_the_launch(family):
    r, n = 128, SMALL_N[family] if family in ("pointnet2", "pointconv") else 256
    model, _ = probes.coalition_model(family, DEV)
    clouds, centers = _clouds(n, first=2)
    rng = np.random.default_rng(11)
    rid = hip_ops.as_i32(rng.integers(0, r, size=(1, n)), DEV)
    member = rng.random((200, 128)) < rng.random((200, 1))
    weights = np.left_shift(np.uint64(1), (np.arange(128) & 63).astype(np.uint64))
    rows = np.where(member, weights, np.uint64(0)).reshape(200, 2, 64).sum(axis=2, dtype=np.uint64)
    kw = hip_ops.wide_masks_to_tensor(rows, DEV)
    big = model.coalition_logits_wide(clouds, centers, rid, kw, None, num_regions=r).clone()
    if family == "pointconv":       # a second call on the same clouds re-uses the cached tables
        assert model.engine()._tab.get("state", 0) != 0
        assert torch.equal(model.coalition_logits_wide(clouds, centers, rid, kw, None, num_regions=r), big)
    # one coalition alone (DGCNN / GCNN: its layer-1 graph then comes from knn_kernel instead of the list walk - the same neighbours)
    assert torch.equal(model.coalition_logits_wide(clouds, centers, rid, kw[77:78].contiguous(), None, num_regions=r), big[77:78])
    cap = type(model).max_clouds_per_call
    try:
        type(model).max_clouds_per_call = 64
        assert torch.equal(model.coalition_logits_wide(clouds, centers, rid, kw, None, num_regions=r), big)
    finally:
        type(model).max_clouds_per_call = cap


# ---- 6. the API ----

def _norm_rel(got, want):
    return float(np.linalg.norm(np.asarray(got) - np.asarray(want)) / np.linalg.norm(np.asarray(want)))


@pytest.mark.parametrize("family", ["gcnn", "pointnet2"])
def test_shapley_compact_at_128_regions(family):
    r, perms = 128, 6
    n = 256 if family == "gcnn" else 128
    model, _ = probes.coalition_model(family, DEV)
    pts, y = synth.make_cloud(0, n)
    data, lbl = torch.from_numpy(pts)[None].to(DEV), torch.tensor([y]).to(DEV)
    rng = np.random.default_rng(13)
    rid = rng.integers(0, r, size=n)
    rid[:r] = np.arange(r)
    orders = synth.make_orders(perms, r, seed=5)
    args = _args(family, r, n)
    _, rows, total = wide.shapley(model, data, lbl, rid, orders, args, coalitions="compact")
    assert rows.shape == (perms, r) and rows.dtype == np.float64 and total.shape == (r,)
    # the rows from coalition_logits on the prefix masks: the same bits
    logits = wide.coalition_logits(model, data, rid, wide.prefix_keep_masks(orders, r), args, coalitions="compact")
    v = final_common.get_reward(logits, lbl, args)
    _, rows2, _ = hip_ops.shapley_snapshots(v, hip_ops.as_i32(orders, DEV), None, hip_ops.shapley_accum_wide)
    assert np.array_equal(rows, rows2)
    assert torch.equal(wide.prefix_logits(model, data, rid, orders, args, coalitions="compact"), logits)
    # efficiency: R float32 roundings of at most 2 max|v| 2^-24 each
    vh = v.cpu().numpy().reshape(perms, r + 1).astype(np.float64)
    bound = r * 2 * float(np.abs(vh).max()) * 2.0 ** -24
    gap = np.array([abs(math.fsum(list(row) + [-vs[-1], vs[0]])) for row, vs in zip(rows, vh)])
    print("%s efficiency: worst gap / bound = %.3g" % (family, float(gap.max() / bound)))
    assert np.all(gap <= bound), (gap, bound)
    _, rows_dense, total_dense = wide.shapley(model, data, lbl, rid, orders, args, coalitions="dense")
    e_rows, e_total = _norm_rel(rows, rows_dense), _norm_rel(total, total_dense)
    print("%s R=128 compact vs dense: rows rel %.3g, total rel %.3g" % (family, e_rows, e_total))
    assert e_rows <= 1e-4 and e_total <= 1e-4


@pytest.mark.parametrize("family", ["gcnn", "pointconv"])
def test_interaction_logits_compact(family):
    r, n = 128, 256
    model, _ = probes.coalition_model(family, DEV)
    pts, _ = synth.make_cloud(1, n)
    data = torch.from_numpy(pts)[None].to(DEV)
    rng = np.random.default_rng(17)
    rid = rng.integers(0, r, size=n)
    rid[:r] = np.arange(r)
    pairs = np.array([[3, 100], [64, 127]])
    args = _args(family, r, n)
    for m in (0, (r - 2) // 2, r - 2):
        ctx = np.stack([np.stack([rng.permutation(np.setdiff1d(np.arange(r), p))[:m] for _ in range(3)]) for p in pairs])
        got = wide.interaction_logits(model, data, rid, pairs, ctx.reshape(2, 3, m), args, coalitions="compact")
        assert got.shape == (2, 12, 10) and torch.isfinite(got).all()
        keep = wide.context_keep_masks(pairs, ctx.reshape(2, 3, m), r)
        want = wide.coalition_logits(model, data, rid, keep, args, coalitions="compact")
        assert torch.equal(got.reshape(24, 10), want)
        dense = wide.interaction_logits(model, data, rid, pairs, ctx.reshape(2, 3, m), args)
        assert probes.rel_max_err(got.cpu().numpy(), dense.cpu().numpy()) < 2e-5


@pytest.mark.parametrize("family", FAMILIES)
def test_dense_and_none_are_the_dense_forward_bitwise(family):
    r, n = 128, 256
    model, _ = probes.coalition_model(family, DEV)
    pts, _ = synth.make_cloud(1, n)
    d = torch.from_numpy(pts)[None].to(DEV)
    rng = np.random.default_rng(19)
    rid = rng.integers(0, r, size=n)
    rows = rng.integers(0, 1 << 63, size=(12, 2), dtype=np.uint64)
    masked = hip_ops.mask_coalitions_wide(d[0].contiguous(), hip_ops.as_i32(rid, DEV), hip_ops.wide_masks_to_tensor(rows, DEV),
                                          d.mean(dim=1).reshape(3).contiguous(), r)
    want = model.forward_points(masked).clone()
    args = _args(family, r, n)
    assert torch.equal(wide.coalition_logits(model, d, rid, rows, args, coalitions="dense"), want)
    assert torch.equal(wide.coalition_logits(model, d, rid, rows, args, coalitions=None), want)
    compact = wide.coalition_logits(model, d, rid, rows, args, coalitions="compact")
    assert probes.rel_max_err(compact.cpu().numpy(), want.cpu().numpy()) < 2e-5


def test_pointnet_compact_is_its_fused_path():
    r = 128
    model, _ = probes.coalition_model("pointnet", DEV)
    pts, _ = synth.make_cloud(1, 256)
    d = torch.from_numpy(pts)[None].to(DEV)
    rng = np.random.default_rng(23)
    rid = rng.integers(0, r, size=256)
    rows = rng.integers(0, 1 << 63, size=(9, 2), dtype=np.uint64)
    args = _args("pointnet", r, 256)
    assert torch.equal(wide.coalition_logits(model, d, rid, rows, args, coalitions="compact"), wide.coalition_logits(model, d, rid, rows, args))


def test_compact_error_paths():
    model, _ = probes.coalition_model("pointconv", DEV)
    pts, _ = synth.make_cloud(0, 2048)
    d = torch.from_numpy(pts)[None].to(DEV)
    rid = np.arange(2048) % 128
    rows = np.ones((2, 2), dtype=np.uint64)
    args = _args("pointconv", 128, 2048)
    with pytest.raises(_lib.IqError):
        wide.coalition_logits(model, d, rid, rows, args, coalitions="fast")
    with pytest.raises(_lib.IqError):
        wide.coalition_logits(model, d, rid, rows, args, coalitions="compact")     # PointConv's compact path stops at 1024 points
    pn2, _ = probes.coalition_model("pointnet2", DEV)
    with pytest.raises(_lib.IqError):
        wide.coalition_logits(pn2, d, rid, rows, _args("pointnet2", 128, 2048), coalitions="compact")
    assert wide.coalition_logits(model, d, rid, rows, args, coalitions="dense").shape == (2, 10)   # the dense route takes the cloud


# ---- 7. the driver ----

def test_final_wide_shapley_compact_writes_the_same_artefacts(tmp_path):
    import gc
    gc.collect()
    torch.cuda.empty_cache()            # the child shares this GPU: hand back what the caching allocator holds
    env = dict(os.environ, PYTHONPATH=REPO)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "IQ_FORCE_DIST", "IQ_REHEARSAL"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(REPO, "final_wide_shapley.py"), "--model", "gcnn", "--dataset", "modelnet10", "--synthetic",
           "--num_clouds", "1", "--num_samples_save", "2", "--num_regions", "128", "--coalitions", "compact"]
    res = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-3000:]
    # the names, shapes and dtypes of a run without the flag (tests/test_wide_gpu.py: test_final_wide_shapley_script_end_to_end)
    root = tmp_path / "checkpoints" / "exp_MODEL_gcnn_DATA_modelnet10_POINTNUM_1024_REGIONNUM_128_shapley_test" / "synthetic_00"
    region_id, all_orders = np.load(root / "region_id.npy"), np.load(root / "all_orders.npy")
    sv = np.load(root / "region_sv_all.npy")
    assert region_id.shape == (1024,) and region_id.dtype == np.int64 and region_id.min() == 0 and region_id.max() == 127
    assert np.load(root / "norm_factor.npy").shape == ()
    assert all_orders.shape == (2, 128) and np.array_equal(all_orders, synth.make_orders(2, 128, seed=1))
    assert sv.shape == (2, 128) and sv.dtype == np.float64
    assert (tmp_path / "fps_modelnet10_1024_128_index_final30.npy").exists()
    # the API with coalitions="compact" on the same cloud, regions and permutations: the same bits
    pts, y = synth.make_cloud(0)
    model, _ = probes.coalition_model("gcnn", DEV)
    _, rows, _ = wide.shapley(model, torch.from_numpy(pts)[None].to(DEV), torch.tensor([y]).to(DEV), region_id, all_orders,
                              _args("gcnn", 128), coalitions="compact")
    assert np.array_equal(rows, sv)
