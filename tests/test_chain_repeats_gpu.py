"""GPU: repeated coalitions in one batch of PointNet keep masks.  A Shapley sample repeats far more than its full and empty sets
(1000 one-region prefixes are at most R distinct sets), so the library finds, on the device, the first item of every (cloud, kept
regions) of a batch (pn_rep_insert_kernel, pn_rep_write_kernel), the chain kernels compute only those and the others take their
pooled rows (pn_dup_copy_kernel).  Logits, feature transforms and arg-max rows must equal, bit for bit, what the twin that computes
every item gives (the twin "chain_no_dedup") and what an item gives alone; the representatives themselves
(iq_debug_pointnet_reps) must be NumPy's first occurrences, exactly."""
import numpy as np
import pytest
import torch

import probes
from interpret_quality_amd import _lib, hip_ops, pointnet, synth, tuning

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
R = 8
BIG = pointnet.ORDER_FUSED_MAX + 1
_INPUTS = {}


def _inputs(n, r=R, nc=1, stray=False):
    """nc synthetic clouds of n points, their centres, region ids drawn at random over r regions."""
    key = (n, r, nc, stray)
    if key not in _INPUTS:
        rng = np.random.default_rng(17 + n + r)
        pts = np.stack([synth.make_cloud(3 + c, max(n, 1024))[0][:n] for c in range(nc)])
        rid = rng.integers(0, r, size=(nc, n))
        if stray:                 # a point outside every region: no mask keeps it, so every item carries a centre row
            rid[:, n // 2] = r + 5
        clouds = torch.from_numpy(pts).to(DEV).contiguous()
        _INPUTS[key] = (clouds, clouds.mean(dim=1).contiguous(), hip_ops.as_i32(rid, DEV))
    return _INPUTS[key]


def _run(inputs, masks, r=R, cloud_of=None, twin=None):
    model, _ = probes.coalition_model("pointnet", DEV)
    clouds, centers, rid = inputs
    keep = hip_ops.masks_to_tensor(np.asarray(masks, dtype=np.uint64), DEV)
    names = None if cloud_of is None else hip_ops.as_i32(np.asarray(cloud_of, dtype=np.int64), DEV)
    with tuning.twin(twin):
        return model.engine().coalition_logits(clouds, centers, rid, keep, names, num_regions=r, return_trans_feat=True, return_crt=True)


_same = probes.same_tensors


def _rows(out, idx):
    return [t[idx] for t in out]


def _first_occurrence(masks, r, cloud_of=None):
    """rep[i] = the lowest j with the same cloud and the same low r bits of the mask."""
    full = np.uint64(0xFFFFFFFFFFFFFFFF) if r >= 64 else np.uint64((1 << r) - 1)
    m = np.asarray(masks, dtype=np.uint64) & full
    c = np.zeros(len(m), dtype=np.uint64) if cloud_of is None else np.asarray(cloud_of).astype(np.uint64)
    _, first, inv = np.unique(np.stack([c, m], axis=1), axis=0, return_index=True, return_inverse=True)
    return first[inv.reshape(-1)].astype(np.int32)


def _pool(rng):
    """A few distinct masks of every density: the empty set, two of 1 .. 7 regions each where they differ, the full set."""
    pool = {0, (1 << R) - 1}
    for d in range(1, R):
        for _ in range(2):
            pool.add(int(sum(1 << int(i) for i in rng.choice(R, size=d, replace=False))))
    return np.array(sorted(pool), dtype=np.uint64)


def _pooled_batch(b, seed=0):
    """b masks from the pool; from 37 items on every mask of the pool occurs at least twice, anywhere.  b = 2: one mask twice."""
    rng = np.random.default_rng(100 + b + seed)
    pool = _pool(rng)
    if b < 2 * len(pool):
        return np.repeat(pool[rng.integers(len(pool))], b)
    masks = np.concatenate([pool, pool, pool[rng.integers(len(pool), size=b - 2 * len(pool))]])
    rng.shuffle(masks)
    return masks


def _distinct_batch(b, r=16):
    return np.random.default_rng(5).choice(1 << r, size=b, replace=False).astype(np.uint64)


def _cloud_batch(b=60, nc=3):
    rng = np.random.default_rng(23)
    pool = _pool(rng)[::3]                                  # few masks, so that each meets every cloud several times
    return pool[rng.integers(len(pool), size=b)], rng.integers(0, nc, size=b)


def _high_bit_batch():
    """Masks that differ only in bits at and above R, among others."""
    base = np.array([0x35, 0x35 | (0xAB << R), 0x35 | (1 << 63), 0xFF, 0xFF | (1 << R), 0, 1 << 40, 0x36, 0x35], dtype=np.uint64)
    return base


def _check_twin_and_alone(inputs, masks, r=R, alone=()):
    got = _run(inputs, masks, r)
    assert got[0].shape == (len(masks), 10) and torch.isfinite(got[0]).all()
    assert _same(got, _run(inputs, masks, r, twin="chain_no_dedup"))
    for i in alone:
        assert _same(_rows(got, slice(i, i + 1)), _run(inputs, masks[i:i + 1], r)), i
    return got


@pytest.mark.parametrize("n,b", [(200, 2), (200, 37), (1024, 37), (200, pointnet.ORDER_FUSED_MAX), (200, BIG)])
def test_repeated_masks_equal_the_twin_and_the_item_alone(n, b):
    masks = _pooled_batch(b)
    rep = _first_occurrence(masks, R)
    copies = np.flatnonzero(rep != np.arange(b))
    assert len(copies) >= b // 2 and rep[0] == 0
    a_rep = int(rep[copies[len(copies) // 2]])              # a representative that has copies: not only item 0
    _check_twin_and_alone(_inputs(n), masks, alone={a_rep, int(copies[0]), int(copies[-1]), b - 1})


def test_one_mask_in_every_item():
    masks = np.full(BIG, 0x5A, dtype=np.uint64)
    got = _check_twin_and_alone(_inputs(200), masks)
    assert all(bool((t == t[0]).all()) for t in got)


def test_all_masks_distinct():
    """R = 16 (R = 8 has only 256 masks): nothing repeats, the table of representatives holds BIG keys at its design load."""
    _check_twin_and_alone(_inputs(200, r=16), _distinct_batch(BIG), r=16)


def test_several_clouds_share_rows_only_inside_a_cloud():
    nc = 3
    masks, cloud_of = _cloud_batch(nc=nc)
    inputs = _inputs(200, nc=nc)
    got = _run(inputs, masks, cloud_of=cloud_of)
    assert _same(got, _run(inputs, masks, cloud_of=cloud_of, twin="chain_no_dedup"))
    for c in range(nc):                                     # the same mask on another cloud is another coalition
        sel = np.flatnonzero(cloud_of == c)
        one = tuple(t[c:c + 1].contiguous() for t in inputs)
        assert _same(_rows(got, torch.from_numpy(sel).to(DEV)), _run(one, masks[sel])), c
    rep = _first_occurrence(masks, R, cloud_of)
    assert (rep != np.arange(len(masks))).sum() >= len(masks) // 2
    assert _same(got, _rows(got, torch.from_numpy(rep.astype(np.int64)).to(DEV)))   # the same mask on the same cloud: one row
    other = int(np.flatnonzero((masks == masks[0]) & (cloud_of != cloud_of[0]))[0])
    assert not torch.equal(got[0][0], got[0][other])        # ... and the same mask on another cloud gives another row


def test_mask_bits_at_and_above_r_name_no_region():
    masks = _high_bit_batch()
    got = _check_twin_and_alone(_inputs(200), masks, alone=range(len(masks)))
    assert _same(_rows(got, slice(0, 1)), _rows(got, slice(1, 2))) and _same(_rows(got, slice(0, 1)), _rows(got, slice(2, 3)))


def _r64_batch():
    masks = np.full(5, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    masks[3] = 0x7FFFFFFFFFFFFFFF                            # bit 63 is a region at R = 64
    return masks


def test_r64_full_masks():
    masks = _r64_batch()
    got = _check_twin_and_alone(_inputs(200, r=64), masks, r=64, alone={3, 4})
    assert _same(_rows(got, slice(0, 1)), _rows(got, slice(4, 5)))


def test_repeated_masks_over_a_stray_point():
    masks = _pooled_batch(37, seed=1)
    _check_twin_and_alone(_inputs(200, stray=True), masks)


def _rep_cases():
    cases = [("pool-%d" % b, _pooled_batch(b), None, R) for b in (2, 37, pointnet.ORDER_FUSED_MAX, BIG)]
    cases.append(("one-mask", np.full(BIG, 0x5A, dtype=np.uint64), None, R))
    cases.append(("distinct", _distinct_batch(BIG), None, 16))
    masks, cloud_of = _cloud_batch()
    cases.append(("clouds", masks, cloud_of, R))
    cases.append(("high-bits", _high_bit_batch(), None, R))
    cases.append(("r64", _r64_batch(), None, 64))
    return cases


@pytest.mark.parametrize("name,masks,cloud_of,r", _rep_cases(), ids=[c[0] for c in _rep_cases()])
def test_representatives_are_the_first_occurrences(name, masks, cloud_of, r):
    keep = hip_ops.masks_to_tensor(masks, DEV)
    names = None if cloud_of is None else hip_ops.as_i32(np.asarray(cloud_of, dtype=np.int64), DEV)
    nc = 1 if cloud_of is None else int(cloud_of.max()) + 1
    rep = hip_ops.pointnet_reps(keep, names, num_regions=r, nclouds=nc).cpu().numpy()
    assert np.array_equal(rep, _first_occurrence(masks, r, cloud_of))
    assert (rep <= np.arange(len(rep))).all() and np.array_equal(rep[rep], rep)


def test_too_small_a_scratch_is_refused():
    keep = hip_ops.masks_to_tensor(_pooled_batch(37), DEV)
    need = 4 * 128                                          # the smallest power of two >= 2 * 37 slots of int32
    assert hip_ops.pointnet_reps(keep, scratch_bytes=need).shape == (37,)
    with pytest.raises(_lib.IqError, match=r"iq_debug_pointnet_reps failed \(-3\): iq_debug_pointnet_reps: scratch") as err:
        hip_ops.pointnet_reps(keep, scratch_bytes=need - 4)
    assert b"iq_debug_pointnet_reps" in _lib.load().iq_last_error()
    assert "%d < %d" % (need - 4, need) in str(err.value)
