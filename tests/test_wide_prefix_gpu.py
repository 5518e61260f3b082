"""GPU: the prefix coalitions of wide games straight from the permutations (iq_pointnet_prefix_coalitions_wide,
PointNetCls.prefix_logits_wide, wide.prefix_logits, wide.shapley(route=...)).

Bars (none is new):
  * the reference of every bitwise test is the existing keep route on hip_ops.prefix_keep_masks_wide(orders): logits and the packed
    feature transform agree bit for bit (a row list holds the same points in another order and every pooling is an exact maximum);
    at R <= 64 the reference is the NARROW coalition_logits on hip_ops.prefix_keep_masks(orders);
  * logits against the CPU oracle: 1e-4 element-wise (conftest.assert_close_elementwise), as everywhere for PointNet.
"""
import argparse
import ctypes

import numpy as np
import pytest
import torch

import probes
from conftest import assert_close_elementwise
from interpret_quality_amd import _lib, hip_ops, synth, wide
from interpret_quality_amd.engine import ptr, stream

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _args(family="pointnet", num_regions=128, num_points=1024):
    return argparse.Namespace(model=family, softmax_type="modified", num_points=num_points, num_regions=num_regions, verbose=False)


def _cloud(i, n=1024):
    pts, y = synth.make_cloud(i, n)
    return torch.from_numpy(pts)[None], torch.tensor([y])


def _inputs(rid, n, cloud_ids=(0,)):
    """clouds (nc,n,3), centers (nc,3) and region ids (nc,n) int32 on the device; ``rid`` (n,) or (nc,n) host ids."""
    clouds = torch.cat([_cloud(i, n)[0] for i in cloud_ids], dim=0)
    rid = np.array(np.broadcast_to(np.asarray(rid).reshape(-1, n), (len(cloud_ids), n)))
    return clouds.to(DEV).contiguous(), clouds.mean(dim=1).to(DEV).contiguous(), hip_ops.as_i32(rid, DEV)


def _perms(rng, s, r):
    return np.stack([rng.permutation(r) for _ in range(s)])


def _both(clouds, centers, rid, orders, r, cloud_of=None, item_cloud_of=None):
    """(logits, packed trans_feat) of the prefix route and of the keep route on the same permutations, engine level."""
    eng = probes.coalition_model("pointnet", DEV)[0].engine()
    od = hip_ops.as_i32(orders, DEV)
    got = eng.prefix_logits_wide(clouds, centers, rid, od, cloud_of, num_regions=r, return_trans_feat=True)
    want = eng.coalition_logits_wide(clouds, centers, rid, hip_ops.prefix_keep_masks_wide(od), item_cloud_of, num_regions=r,
                                     return_trans_feat=True)
    return got, want


def _assert_same(got, want):
    assert got[0].shape == want[0].shape and got[1].shape == want[1].shape
    assert torch.isfinite(got[0]).all()
    assert torch.equal(got[0], want[0]), "logits differ in %d rows" % int((got[0] != want[0]).any(dim=1).sum())
    assert torch.equal(got[1], want[1]), "trans_feat differs in %d rows" % int((got[1] != want[1]).any(dim=1).sum())


# ---- 1. prefix = keep, bitwise ----

@pytest.mark.parametrize("n,r,per_point", [(1024, 65, False), (1024, 128, False), (1000, 200, False), (256, 256, True),
                                           (1024, 1024, True), (2500, 1024, False)])
def test_prefix_route_equals_keep_route_bitwise(n, r, per_point):
    rng = np.random.default_rng(1000 * r + n)
    rid = rng.permutation(n) if per_point else rng.integers(0, r, size=n)
    clouds, centers, ridt = _inputs(rid, n)
    got, want = _both(clouds, centers, ridt, _perms(rng, 3, r), r)
    assert got[0].shape == (3 * (r + 1), 10) and got[1].shape == (3 * (r + 1), 4096)
    _assert_same(got, want)


# ---- 2. crafted regions ----

def test_crafted_regions_long_copy_empty_regions_and_a_full_item_before_the_end():
    n, r = 1024, 70
    rng = np.random.default_rng(70)
    rid = np.empty(n, dtype=np.int64)
    rid[:300] = 0                                              # one region of 300 points: a copy longer than a wave
    rest = np.array([q for q in range(1, r) if q not in (5, 6)])   # regions 5 and 6 are empty
    rid[300:] = rest[rng.integers(0, len(rest), size=n - 300)]
    rid = rid[rng.permutation(n)]
    orders = _perms(rng, 3, r)
    o0 = [q for q in orders[0] if q not in (5, 6)]
    orders[0] = o0[:20] + [5, 6] + o0[20:]                     # items 20, 21 and 22 keep the same points
    orders[1] = [q for q in orders[1] if q != 6] + [6]         # an empty region last: item R - 1 is already full (no centre)
    clouds, centers, ridt = _inputs(rid, n)
    got, want = _both(clouds, centers, ridt, orders, r)
    _assert_same(got, want)
    for t in got:
        assert torch.equal(t[20], t[21]) and torch.equal(t[21], t[22])
        assert torch.equal(t[(r + 1) + r - 1], t[(r + 1) + r])
        assert not torch.equal(t[19], t[20])
    # the empty prefix (the centre alone) against the all-zero keep row evaluated alone
    eng = probes.coalition_model("pointnet", DEV)[0].engine()
    zero = torch.zeros((1, 2), dtype=torch.int64, device=DEV)
    alone = eng.coalition_logits_wide(clouds, centers, ridt, zero, None, num_regions=r, return_trans_feat=True)
    for o in range(3):
        assert torch.equal(got[0][o * (r + 1)], alone[0][0]) and torch.equal(got[1][o * (r + 1)], alone[1][0])


# ---- 3. malformed permutations: such entries are ignored by specification ----

def test_out_of_range_and_repeated_entries_are_ignored_as_the_keep_route_ignores_them():
    n, r = 1024, 128
    rng = np.random.default_rng(3)
    orders = _perms(rng, 3, r)
    orders[0][r // 3] = r + 5                                  # out of range: its region is never kept
    orders[1][50] = orders[1][10]                              # a region twice, hence one region missing
    orders[2][7] = -3
    clouds, centers, ridt = _inputs(rng.integers(0, r, size=n), n)
    got, want = _both(clouds, centers, ridt, orders, r)
    _assert_same(got, want)
    assert torch.equal(got[0][(r + 1) + 50], got[0][(r + 1) + 51])   # the repeated entry added nothing
    assert torch.isfinite(got[0]).all() and torch.isfinite(got[1]).all()


# ---- 4. R <= 64: the narrow path's bits ----

@pytest.mark.parametrize("r", [32, 64])
def test_prefix_route_equals_the_narrow_path_bitwise_up_to_64_regions(r):
    n = 1024
    rng = np.random.default_rng(r)
    model, _ = probes.coalition_model("pointnet", DEV)
    clouds, centers, ridt = _inputs(rng.integers(0, r, size=n), n)
    od = hip_ops.as_i32(_perms(rng, 3, r), DEV)
    narrow = model.coalition_logits(clouds, centers, ridt, hip_ops.prefix_keep_masks(od), None, num_regions=r)
    got = model.prefix_logits_wide(clouds, centers, ridt, od, None, num_regions=r)
    assert got.shape == (3 * (r + 1), 10) and torch.equal(got, narrow)


# ---- 5. two clouds, a cloud per permutation ----

@pytest.mark.parametrize("pose_like", [False, True])
def test_cloud_of_names_a_cloud_per_permutation(pose_like):
    n, r, s = 1024, 128, 4
    rng = np.random.default_rng(5 + pose_like)
    if pose_like:                                              # cloud 1 is cloud 0 translated; both share the region ids
        clouds, _, ridt = _inputs(rng.integers(0, r, size=n), n, cloud_ids=(0, 0))
        clouds[1] += torch.tensor([0.25, -0.5, 0.125], device=DEV)
        centers = clouds.mean(dim=1).contiguous()
    else:
        clouds, centers, ridt = _inputs(rng.integers(0, r, size=(2, n)), n, cloud_ids=(0, 1))
    orders = _perms(rng, s, r)
    names = [1, 0, 0, 1]
    cloud_of = torch.tensor(names, dtype=torch.int32, device=DEV)
    got, want = _both(clouds, centers, ridt, orders, r, cloud_of, cloud_of.repeat_interleave(r + 1).contiguous())
    _assert_same(got, want)
    eng = probes.coalition_model("pointnet", DEV)[0].engine()
    for o, c in enumerate(names):
        one = eng.prefix_logits_wide(clouds[c:c + 1].contiguous(), centers[c:c + 1].contiguous(), ridt[c:c + 1].contiguous(),
                                     hip_ops.as_i32(orders[o:o + 1], DEV), None, num_regions=r, return_trans_feat=True)
        blk = slice(o * (r + 1), (o + 1) * (r + 1))
        assert torch.equal(got[0][blk], one[0]) and torch.equal(got[1][blk], one[1])
    assert not torch.equal(got[0][:r + 1], got[0][(r + 1):2 * (r + 1)])
    # one cloud per permutation needs no cloud_of
    two = eng.prefix_logits_wide(clouds, centers, ridt, hip_ops.as_i32(orders[:2], DEV), None, num_regions=r)
    pair = eng.prefix_logits_wide(clouds, centers, ridt, hip_ops.as_i32(orders[:2], DEV),
                                  torch.tensor([0, 1], dtype=torch.int32, device=DEV), num_regions=r)
    assert torch.equal(two, pair)


# ---- 6. launch independence ----

def test_prefix_logits_do_not_depend_on_the_launch(monkeypatch):
    n, r, s = 1024, 128, 5
    rng = np.random.default_rng(6)
    model, _ = probes.coalition_model("pointnet", DEV)
    clouds, centers, ridt = _inputs(rng.integers(0, r, size=n), n)
    od = hip_ops.as_i32(_perms(rng, s, r), DEV)
    big = model.prefix_logits_wide(clouds, centers, ridt, od, None, num_regions=r)
    sizes = []
    eng = model.engine()
    launch = eng.prefix_logits_wide
    monkeypatch.setattr(eng, "prefix_logits_wide", lambda c, ce, ri, o, *a, **k: (sizes.append(o.shape[0]), launch(c, ce, ri, o, *a, **k))[1])
    monkeypatch.setattr(type(model), "max_wide_per_call", 2 * (r + 1) + 17)
    split = model.prefix_logits_wide(clouds, centers, ridt, od, None, num_regions=r)
    assert sizes == [2, 2, 1]
    assert big.shape == (s * (r + 1), 10) and torch.equal(split, big)
    monkeypatch.setattr(type(model), "max_wide_per_call", 5)      # fewer coalitions than a permutation has: one permutation a launch
    del sizes[:]
    assert torch.equal(model.prefix_logits_wide(clouds, centers, ridt, od[:2].contiguous(), None, num_regions=r), big[:2 * (r + 1)])
    assert sizes == [1, 1]


# ---- 7. the oracle ----

def test_prefix_logits_match_the_oracle():
    n, r, s = 1024, 128, 2
    rng = np.random.default_rng(7)
    model, sd = probes.coalition_model("pointnet", DEV)
    rid = rng.integers(0, r, size=n)
    clouds, centers, ridt = _inputs(rid, n)
    orders = _perms(rng, s, r)
    got = model.prefix_logits_wide(clouds, centers, ridt, hip_ops.as_i32(orders, DEV), None, num_regions=r).cpu().numpy()
    kept = np.stack([np.isin(rid, orders[o][:i]) for o in range(s) for i in range(r + 1)])
    pts, c = clouds[0].cpu(), centers[0].cpu()
    b = s * (r + 1)
    masked = torch.where(torch.from_numpy(kept)[:, :, None], pts[None].expand(b, n, 3), c.reshape(1, 1, 3).expand(b, n, 3)).contiguous()
    want = probes.oracle_logits("pointnet", sd, masked)
    print("prefix route R=128 vs oracle: max |d| / max |logit| = %.3g" % probes.rel_max_err(got, want))
    assert_close_elementwise(got, want, rtol=1e-4)


# ---- 8. wide.shapley and wide.prefix_logits ----

@pytest.mark.parametrize("n,r,s", [(1024, 128, 6), (256, 256, 2)])
def test_shapley_prefix_route_gives_the_keep_route_bits(n, r, s):
    rng = np.random.default_rng(8 + r)
    data, lbl = _cloud(0, n)
    rid = rng.permutation(n) if r == n else rng.integers(0, r, size=n)
    orders = synth.make_orders(s, r, seed=5)
    model, _ = probes.coalition_model("pointnet", DEV)
    args = _args("pointnet", r, n)
    res = {route: wide.shapley(model, data.to(DEV), lbl.to(DEV), rid, orders, args, snap_counts=[s // 2, s], perms_per_step=max(1, s // 2),
                               route=route) for route in ("keep", "prefix", None)}
    for route in ("prefix", None):
        snaps, rows, total = res[route]
        assert sorted(snaps) == [s // 2, s] and all(np.array_equal(snaps[k], res["keep"][0][k]) for k in snaps)
        assert rows.shape == (s, r) and np.array_equal(rows, res["keep"][1]) and np.array_equal(total, res["keep"][2])
    assert np.isfinite(res["prefix"][1]).all() and np.count_nonzero(res["prefix"][1]) > r


def test_a_family_without_the_entry_refuses_the_prefix_route_and_takes_the_keep_rows():
    n, r = 256, 65
    rng = np.random.default_rng(9)
    model, _ = probes.coalition_model("pointnet2", DEV)
    assert not hasattr(model, "prefix_logits_wide")
    data, lbl = _cloud(1, n)
    rid = rng.integers(0, r, size=n)
    orders = _perms(rng, 1, r)
    args = _args("pointnet2", r, n)
    with pytest.raises(_lib.IqError):
        wide.shapley(model, data.to(DEV), lbl.to(DEV), rid, orders, args, route="prefix")
    got = wide.prefix_logits(model, data.to(DEV), rid, orders, args)
    want = wide.coalition_logits(model, data.to(DEV), rid, hip_ops.prefix_keep_masks_wide(hip_ops.as_i32(orders, DEV)), args)
    assert got.shape == (r + 1, 10) and torch.equal(got, want)


def test_public_prefix_logits_on_pointnet_equals_coalition_logits():
    n, r = 1024, 128
    rng = np.random.default_rng(10)
    model, _ = probes.coalition_model("pointnet", DEV)
    data, _ = _cloud(2, n)
    rid = rng.integers(0, r, size=n)
    orders = _perms(rng, 2, r)
    args = _args("pointnet", r, n)
    got = wide.prefix_logits(model, data.to(DEV), rid, orders, args)
    want = wide.coalition_logits(model, data.to(DEV), rid, wide.prefix_keep_masks(orders, r), args)
    assert got.shape == (2 * (r + 1), 10) and torch.equal(got, want)


# ---- 9. argument checks ----

def test_prefix_entry_refuses_bad_arguments():
    n, r = 1024, 128
    rng = np.random.default_rng(11)
    model, _ = probes.coalition_model("pointnet", DEV)
    eng = model.engine()
    clouds, centers, ridt = _inputs(rng.integers(0, r, size=(2, n)), n, cloud_ids=(0, 1))
    one = (clouds[:1].contiguous(), centers[:1].contiguous(), ridt[:1].contiguous())
    od = hip_ops.as_i32(_perms(rng, 3, r), DEV)
    with pytest.raises(_lib.IqError):
        model.prefix_logits_wide(*one, torch.zeros((1, 1025), dtype=torch.int32, device=DEV), None, num_regions=1025)
    with pytest.raises(_lib.IqError):
        model.prefix_logits_wide(*one, od[:, :r - 1].contiguous(), None, num_regions=r)          # orders of the wrong width
    with pytest.raises(_lib.IqError):
        model.prefix_logits_wide(*one, od.cpu(), None, num_regions=r, validate=False)            # a CPU tensor
    with pytest.raises(_lib.IqError):
        model.prefix_logits_wide(clouds, centers, ridt, od, None, num_regions=r)                 # 3 permutations of 2 clouds: whose?
    with pytest.raises(_lib.IqError):
        eng.prefix_logits_wide(clouds, centers, ridt, od, None, num_regions=r)
    # a workspace one byte short, through the raw binding (also R = 1025 and the missing cloud_of: the library's own checks)
    lib, b = eng.lib, 3 * (r + 1)
    need = lib.iq_pointnet_wide_workspace_bytes(b, 1, n, r)
    ws = torch.empty((need,), dtype=torch.uint8, device=DEV)
    logits = torch.empty((b, 10), dtype=torch.float32, device=DEV)

    def raw(nbytes, rr=r, nc=1, cloud_of=None):
        return lib.iq_pointnet_prefix_coalitions_wide(ctypes.byref(eng.weights.struct), ptr(clouds), ptr(centers), ptr(ridt), ptr(od),
                                                      ptr(cloud_of), ptr(logits), ptr(None), ptr(ws), nbytes, 3, nc, n, rr, stream())
    assert raw(need - 1) == -3 and b"workspace" in lib.iq_last_error()       # IQ_EWORKSPACE
    with pytest.raises(_lib.IqError):
        _lib.check(raw(need - 1), "iq_pointnet_prefix_coalitions_wide")
    assert raw(need, rr=1025) != 0 and raw(need, nc=2) != 0
    assert raw(need) == 0
    assert torch.equal(logits, eng.prefix_logits_wide(*one, od, None, num_regions=r))
