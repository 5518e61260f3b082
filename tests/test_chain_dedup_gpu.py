"""GPU: repeated full and empty sets in one batch of PointNet coalitions.  Every permutation of a Shapley sample brings the full and
the empty set once; with one cloud per call the chain kernels compute the first of each kind and the others take its pooled rows
(pn_dup_rep_kernel, pn_dup_copy_kernel).  Logits, feature transforms and arg-max rows must equal, bit for bit, what the twin that
computes every item gives (the twin "chain_no_dedup") and what an item gives alone - wherever the first of a kind stands."""
import numpy as np
import pytest
import torch

import probes
from interpret_quality_amd import hip_ops, pointnet, synth, tuning

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
R = 8
FULL = np.uint64((1 << R) - 1)
_INPUTS = {}


def _inputs(n, stray=False):
    if (n, stray) not in _INPUTS:
        rng = np.random.default_rng(11 + n)
        pts = synth.make_cloud(3, max(n, 1024))[0][:n]
        rid = rng.integers(0, R, size=n)
        if stray:                 # a point outside every region: the "full" mask still masks it, and a centre row appears
            rid[n // 2] = R + 5
        clouds = torch.from_numpy(pts)[None].to(DEV).contiguous()
        _INPUTS[n, stray] = (clouds, clouds.mean(dim=1).contiguous(), hip_ops.as_i32(rid.reshape(1, n), DEV))
    return _INPUTS[n, stray]


def _run(n, masks, twin=None, stray=False):
    model, _ = probes.coalition_model("pointnet", DEV)
    clouds, centers, rid = _inputs(n, stray)
    keep = hip_ops.masks_to_tensor(np.asarray(masks, dtype=np.uint64), DEV)
    with tuning.twin(twin):
        return model.engine().coalition_logits(clouds, centers, rid, keep, None, num_regions=R, return_trans_feat=True, return_crt=True)


def _batch(rng, b, first_full, first_empty):
    """b masks of every density, a third of them full and a third empty from their first positions on."""
    bits = rng.random((b, R)) < rng.random((b, 1))
    bits[:, 0] |= ~bits.any(axis=1)                     # no accidental empty set,
    bits[:, 1] &= ~bits.all(axis=1)                     # no accidental full set
    masks = (bits.astype(np.uint64) << np.arange(R, dtype=np.uint64)).sum(axis=1, dtype=np.uint64)
    kind = rng.integers(0, 3, size=b)
    masks[(kind == 1) & (np.arange(b) >= first_full)] = FULL
    masks[(kind == 2) & (np.arange(b) >= first_empty)] = 0
    if first_full < b:
        masks[first_full] = FULL
    if first_empty < b:
        masks[first_empty] = 0
    return masks


@pytest.mark.parametrize("n", [200, 1024])
@pytest.mark.parametrize("b,first_full,first_empty", [(2, 0, 2), (2, 2, 0), (37, 0, 1), (37, 36, 35), (37, 5, 37), (37, 37, 9),
                                                      (pointnet.ORDER_FUSED_MAX + 1, 4000, 17)])
def test_repeated_sets_equal_the_twin_and_the_item_alone(n, b, first_full, first_empty):
    masks = _batch(np.random.default_rng(b + first_full), b, first_full, first_empty)
    if b == 2:
        masks[:] = FULL if first_full == 0 else 0       # nothing but copies of one item
    got = _run(n, masks)
    assert got[0].shape == (b, 10) and torch.isfinite(got[0]).all()
    assert probes.same_tensors(got, _run(n, masks, twin="chain_no_dedup"))
    for i in {b - 1, b // 2, min(first_full + 1, b - 1), min(first_empty + 1, b - 1)}:     # a copy (or any item) alone
        assert probes.same_tensors([t[i:i + 1] for t in got], _run(n, masks[i:i + 1]))


def test_a_full_mask_over_stray_points_is_no_full_set():
    """With a point outside every region the full mask keeps n - 1 points plus the centre: such items are computed, not copied -
    and still agree with the twin."""
    masks = _batch(np.random.default_rng(3), 21, 2, 4)
    assert probes.same_tensors(_run(200, masks, stray=True), _run(200, masks, twin="chain_no_dedup", stray=True))
