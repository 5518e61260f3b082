"""GPU: the PointNet step on the distinct coalitions of a batch only.  The forward finds the first item of every (cloud, kept regions)
group, moves those U items to slots 0 .. U-1 (pn_compact kernels; U stays on the device), runs row lists, gather, launch order, chains
and heads on the slots, and gives every item its slot's results at the end (pn_expand kernels).  Checked here: the slot map against
NumPy's first occurrences and their ranks (iq_debug_pointnet_slots), and logits, feature transforms and arg-max rows bit for bit
against the twin that evaluates every item in place (twin "chain_no_dedup") and against items run alone - with U on both sides of the
heads' tile heights (32, 64, 128 rows) and of the one-workgroup bound of the order and compaction kernels, with the workspace filled
with NaN patterns beforehand (a read of a row at or past U shows as a NaN or a changed bit), without the optional outputs, and on the
routes that are not compacted."""
import numpy as np
import pytest
import torch

import probes
from interpret_quality_amd import _lib, hip_ops, pointnet, synth, tuning

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
N, R = 200, 8
BIG = pointnet.ORDER_FUSED_MAX + 1
_INPUTS, _RUNS = {}, {}


def _inputs(r=R, nc=1):
    key = (r, nc)
    if key not in _INPUTS:
        rng = np.random.default_rng(31 + r)
        pts = np.stack([synth.make_cloud(5 + c, 1024)[0][:N] for c in range(nc)])
        clouds = torch.from_numpy(pts).to(DEV).contiguous()
        _INPUTS[key] = (clouds, clouds.mean(dim=1).contiguous(), hip_ops.as_i32(rng.integers(0, r, size=(nc, N)), DEV))
    return _INPUTS[key]


def _engine():
    return probes.coalition_model("pointnet", DEV)[0].engine()


def _run(inputs, masks, r=R, cloud_of=None, twin=None, poison=False, tf=True, crt=True):
    """One forward.  ``poison``: in a workspace of exactly the size the library asks for, every byte 0xff (float NaNs, int -1)."""
    eng = _engine()
    clouds, centers, rid = inputs
    keep = hip_ops.masks_to_tensor(np.asarray(masks, dtype=np.uint64), DEV)
    names = None if cloud_of is None else hip_ops.as_i32(np.asarray(cloud_of, dtype=np.int64), DEV)
    if poison:
        need = _lib.load().iq_pointnet_workspace_bytes(len(masks), clouds.shape[0], N, r)
        eng._ws = torch.full((int(need),), 0xFF, dtype=torch.uint8, device=DEV)
    try:
        with tuning.twin(twin):
            out = eng.coalition_logits(clouds, centers, rid, keep, names, num_regions=r, return_trans_feat=tf, return_crt=crt)
            torch.cuda.synchronize()
        return out if isinstance(out, tuple) else (out,)
    finally:
        if poison:
            eng._ws = None


_same = probes.same_tensors


def _reference(masks, r, cloud_of=None):
    """(slot_of, item_u, cloud_u, U): first occurrences of (cloud, low r bits of the mask) and their ranks."""
    full = np.uint64(0xFFFFFFFFFFFFFFFF) if r >= 64 else np.uint64((1 << r) - 1)
    m = np.asarray(masks, dtype=np.uint64) & full
    c = np.zeros(len(m), dtype=np.uint64) if cloud_of is None else np.asarray(cloud_of).astype(np.uint64)
    _, first, inv = np.unique(np.stack([c, m], axis=1), axis=0, return_index=True, return_inverse=True)
    rep = first[inv.reshape(-1)]
    item_u = np.flatnonzero(rep == np.arange(len(m)))
    return np.searchsorted(item_u, rep).astype(np.int32), item_u.astype(np.int32), c[item_u].astype(np.int32), len(item_u)


def _batch(b, u, r=R, seed=0):
    """b masks over r regions, exactly u distinct ones (the empty and the full set among them), every one at least once, shuffled."""
    rng = np.random.default_rng(1000 * b + u + seed)
    inner = rng.choice(np.arange(1, (1 << r) - 1), size=u - 2, replace=False) if u > 2 else np.zeros(0, dtype=np.int64)
    pool = np.concatenate([[0, (1 << r) - 1][:u], inner]).astype(np.uint64)
    masks = np.concatenate([pool, pool[rng.integers(u, size=b - u)]])
    rng.shuffle(masks)
    assert len(np.unique(masks)) == u and len(masks) == b
    return masks


def _map_cases():
    rng = np.random.default_rng(3)
    last = np.arange(1, 41, dtype=np.uint64)
    last[-1] = last[5]
    high = np.array([0x35, 0x35 | (0xAB << R), 0x35 | (1 << 63), 0xFF, 0xFF | (1 << R), 0, 1 << 40, 0x36, 0x35], dtype=np.uint64)
    r64 = np.full(5, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    r64[3] = 0x7FFFFFFFFFFFFFFF
    cmask = _batch(90, 7, seed=9)
    cases = [("all-equal", np.full(77, 0x5A, dtype=np.uint64), None, R),
             ("all-equal-big", np.full(BIG, 0x5A, dtype=np.uint64), None, R),
             ("all-distinct", rng.choice(1 << 16, size=300, replace=False).astype(np.uint64), None, 16),
             ("all-distinct-big", rng.choice(1 << 16, size=BIG, replace=False).astype(np.uint64), None, 16),
             ("repeat-in-last-item", last, None, R),
             ("high-bits", high, None, R),
             ("r64", r64, None, 64),
             ("clouds", cmask, rng.integers(0, 3, size=90), R),
             ("clouds-big", _batch(BIG + 300, 200, seed=2), rng.integers(0, 3, size=BIG + 300), R),
             ("fused-bound", _batch(BIG - 1, 150), None, R),
             ("above-bound", _batch(BIG, 150), None, R)]
    return cases


@pytest.mark.parametrize("name,masks,cloud_of,r", _map_cases(), ids=[c[0] for c in _map_cases()])
def test_slot_map_is_numpys_first_occurrences_and_their_ranks(name, masks, cloud_of, r):
    keep = hip_ops.masks_to_tensor(masks, DEV)
    names = None if cloud_of is None else hip_ops.as_i32(np.asarray(cloud_of, dtype=np.int64), DEV)
    nc = 1 if cloud_of is None else 3
    slot_of, item_u, cloud_u, u = hip_ops.pointnet_slots(keep, names, num_regions=r, nclouds=nc)
    want_slot, want_item, want_cloud, want_u = _reference(masks, r, cloud_of)
    assert u == want_u
    assert np.array_equal(slot_of.cpu().numpy(), want_slot)
    assert np.array_equal(item_u.cpu().numpy(), want_item)
    if cloud_of is not None:
        assert np.array_equal(cloud_u.cpu().numpy(), want_cloud)
        # equal masks on different clouds stay apart
        assert u > len(np.unique(np.asarray(masks) & np.uint64((1 << r) - 1)))
    if name == "all-equal":
        assert u == 1
    if name == "high-bits":
        assert len(set(slot_of.cpu().numpy()[[0, 1, 2, 8]].tolist())) == 1


def _case(b, u, r=R):
    """The compacted run of a batch with its twin-60 run, computed once."""
    key = (b, u, r)
    if key not in _RUNS:
        masks = _batch(b, u, r)
        assert _reference(masks, r)[3] == u
        _RUNS[key] = (masks, _run(_inputs(r), masks, r), _run(_inputs(r), masks, r, twin="chain_no_dedup"))
    return _RUNS[key]


U_CASES = [(u + 40, u, R) for u in (31, 32, 33, 63, 64, 65, 127, 128, 129)] + [(BIG, 200, R), (BIG, BIG, 16)]
U_IDS = ["B%d-U%d" % (b, u) for b, u, _ in U_CASES]


@pytest.mark.parametrize("b,u,r", U_CASES, ids=U_IDS)
def test_results_equal_the_twin_and_items_alone(b, u, r):
    masks, got, twin = _case(b, u, r)
    assert got[0].shape == (b, 10) and got[1].shape == (b, 4096) and got[2].shape == (b, 1024)
    assert torch.isfinite(got[0]).all() and torch.isfinite(got[1]).all()
    assert _same(got, twin)
    slot_of, item_u, _, _ = _reference(masks, r)
    copies = np.flatnonzero(item_u[slot_of] != np.arange(b))
    alone = {int(item_u[-1]), b - 1} | ({int(copies[0]), int(copies[-1])} if len(copies) else set())
    for i in sorted(alone):
        assert _same([t[i:i + 1] for t in got], _run(_inputs(r), masks[i:i + 1], r)), i


@pytest.mark.parametrize("b,u,r", U_CASES, ids=U_IDS)
def test_poisoned_workspace_changes_no_bit(b, u, r):
    masks, got, _ = _case(b, u, r)
    assert _same(got, _run(_inputs(r), masks, r, poison=True))


@pytest.mark.parametrize("b,u,r", [(73, 33, R), (BIG, 200, R)], ids=["B73-U33", "B%d-U200" % BIG])
def test_outputs_not_asked_for(b, u, r):
    """Logits alone, and with each optional output alone, in a poisoned workspace of exactly the reported size."""
    masks, got, _ = _case(b, u, r)
    assert torch.equal(_run(_inputs(r), masks, r, poison=True, tf=False, crt=False)[0], got[0])
    assert _same(_run(_inputs(r), masks, r, poison=True, tf=True, crt=False), got[:2])
    assert _same(_run(_inputs(r), masks, r, poison=True, tf=False, crt=True), (got[0], got[2]))


def test_several_clouds_with_cloud_of():
    rng = np.random.default_rng(41)
    masks, cloud_of = _batch(140, 9, seed=4), rng.integers(0, 3, size=140)
    inputs = _inputs(nc=3)
    got = _run(inputs, masks, cloud_of=cloud_of)
    assert _same(got, _run(inputs, masks, cloud_of=cloud_of, twin="chain_no_dedup"))
    assert _same(got, _run(inputs, masks, cloud_of=cloud_of, poison=True))
    for c in range(3):
        sel = np.flatnonzero(cloud_of == c)
        one = tuple(t[c:c + 1].contiguous() for t in inputs)
        assert _same([t[torch.from_numpy(sel).to(DEV)] for t in got], _run(one, masks[sel])), c


# ---- the routes that are not compacted: the same launches with every item its own slot ------------------------------------------
def _with_twin(fn, twin):
    with tuning.twin(twin):
        out = fn()
        torch.cuda.synchronize()
        return out


def test_wide_entry_at_66_items():
    r = 10
    clouds, centers, rid = _inputs(r)
    masks = _batch(66, 20, r, seed=6)
    keep = hip_ops.masks_to_tensor(masks, DEV).reshape(66, 1).contiguous()
    run = lambda: _engine().coalition_logits_wide(clouds, centers, rid, keep, None, num_regions=r, return_trans_feat=True)
    got = _with_twin(run, None)
    assert _same(got, _with_twin(run, "chain_no_dedup"))
    narrow = _run(_inputs(r), masks, r)                     # the same coalitions through the compacted narrow entry
    assert torch.equal(got[0], narrow[0]) and torch.equal(got[1], narrow[1])


def test_prefix_entry_at_66_items():
    r = 10
    clouds, centers, rid = _inputs(r)
    rng = np.random.default_rng(8)
    orders = hip_ops.as_i32(np.stack([rng.permutation(r) for _ in range(6)]), DEV)
    run = lambda: _engine().prefix_logits_wide(clouds, centers, rid, orders, None, num_regions=r, return_trans_feat=True)
    got = _with_twin(run, None)
    assert got[0].shape == (66, 10) and _same(got, _with_twin(run, "chain_no_dedup"))
    keep = hip_ops.prefix_keep_masks_wide(orders)
    wide = _engine().coalition_logits_wide(clouds, centers, rid, keep, None, num_regions=r, return_trans_feat=True)
    assert _same(got, wide)


def test_a_cloud_per_item_without_cloud_of_at_66_items():
    nc = 66
    rng = np.random.default_rng(12)
    base = _inputs()
    clouds = (base[0] + 0.01 * torch.arange(nc, device=DEV, dtype=torch.float32).reshape(nc, 1, 1)).contiguous()
    inputs = (clouds, clouds.mean(dim=1).contiguous(), hip_ops.as_i32(rng.integers(0, R, size=(nc, N)), DEV))
    masks = _batch(nc, 5, seed=3)                           # equal masks, but every item has a cloud of its own
    got = _run(inputs, masks)
    assert _same(got, _run(inputs, masks, twin="chain_no_dedup"))
    assert _same(got, _run(inputs, masks, poison=True))
    for i in (0, 37, 65):
        one = tuple(t[i:i + 1].contiguous() for t in inputs)
        assert _same([t[i:i + 1] for t in got], _run(one, masks[i:i + 1])), i
