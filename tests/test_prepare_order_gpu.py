"""GPU: the kernels in front of the PointNet chains - the per-cloud region tables (pn_prepare[_wide]_kernel: a stable counting sort
by ballot) and the launch order (one kernel up to pointnet.ORDER_FUSED_MAX coalitions, four above) - through what depends on
them: the logits of a coalition, which must equal the dense forward on its materialised cloud bit for bit, and must not depend
on the order of the batch."""
import numpy as np
import pytest
import torch

import probes
from interpret_quality_amd import final_common, hip_ops, pointnet, synth

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _inputs(n, r, seed, stray=False):
    """A cloud of n points with random region ids in [0, r), region 1 empty (r > 1); ``stray``: two ids outside [0, r), whose
    points every coalition masks."""
    rng = np.random.default_rng(seed)
    pts = synth.make_cloud(seed % 5, max(n, 1024))[0][:n]          # (a synthetic cloud of one point has no scale)
    rid = rng.integers(0, r, size=n)
    if r > 1:
        rid[rid == 1] = 0
    if stray:
        rid[n // 3], rid[n - 1] = r, r + 1000
    clouds = torch.from_numpy(pts)[None].to(DEV).contiguous()
    return clouds, clouds.mean(dim=1).contiguous(), hip_ops.as_i32(rid.reshape(1, n), DEV)


def _masks(rng, b, r):
    """(b,) uint64 masks over r regions: the full set, the empty set, one region alone, then sets of every density."""
    bits = rng.random((b, r)) < rng.random((b, 1))
    bits[0, :], bits[1, :] = True, False
    bits[2, :] = np.arange(r) == r - 1
    return (bits.astype(np.uint64) << np.arange(r, dtype=np.uint64)).sum(axis=1, dtype=np.uint64)


@pytest.mark.parametrize("r", [1, 33, 64])
@pytest.mark.parametrize("n", [1, 70, 1024, 4096])
def test_coalition_logits_equal_the_materialised_forward_bitwise(n, r):
    model, _ = probes.coalition_model("pointnet", DEV)
    clouds, centers, rid = _inputs(n, r, 10 * n + r, stray=n >= 70)
    keep = hip_ops.masks_to_tensor(_masks(np.random.default_rng(n + r), 24, r), DEV)
    got = model.coalition_logits(clouds, centers, rid, keep, None, num_regions=r, validate=False)
    want = final_common.materialised_logits(model, clouds[0].contiguous(), rid[0].contiguous(), keep, centers[0].contiguous(), 24)
    assert got.shape == (24, 10) and torch.isfinite(got).all()
    assert torch.equal(got, want)


def test_wide_coalition_logits_equal_the_materialised_forward_bitwise_at_65_regions():
    model, _ = probes.coalition_model("pointnet", DEV)
    n, r = 1024, 65
    clouds, centers, rid = _inputs(n, r, 65)
    rng = np.random.default_rng(65)
    lo, hi = _masks(rng, 24, 64), rng.integers(0, 2, size=24).astype(np.uint64)      # region 64 is word 1, bit 0
    keep = torch.from_numpy(np.stack([lo, hi], axis=1).view(np.int64)).to(DEV).contiguous()
    got = model.coalition_logits_wide(clouds, centers, rid, keep, None, num_regions=r)
    masked = hip_ops.mask_coalitions_wide(clouds[0].contiguous(), rid[0].contiguous(), keep, centers[0].contiguous(), r, channel_first=True)
    assert torch.equal(got, model(masked)[0])


@pytest.mark.parametrize("b", [1, pointnet.ORDER_FUSED_MAX - 1, pointnet.ORDER_FUSED_MAX, pointnet.ORDER_FUSED_MAX + 1])
def test_logits_do_not_depend_on_the_order_of_the_batch(b):
    """The launch order sorts by row count and is free inside a bin: a coalition's logits are the same wherever it stands.  One
    launch-order kernel up to ORDER_FUSED_MAX coalitions, the four-launch path above."""
    model, _ = probes.coalition_model("pointnet", DEV)
    n, r = 200, 8
    clouds, centers, rid = _inputs(n, r, 7)
    keep = hip_ops.masks_to_tensor(_masks(np.random.default_rng(b), max(b, 3), r)[:b], DEV)
    fwd = model.coalition_logits(clouds, centers, rid, keep, None, num_regions=r, validate=False)
    rev = model.coalition_logits(clouds, centers, rid, keep.flip(0).contiguous(), None, num_regions=r, validate=False)
    assert fwd.shape == (b, 10) and torch.equal(fwd, rev.flip(0))
    if b > 1:       # and they are the logits of the coalitions one by one (a wrong order table would pair rows with other items)
        one = model.coalition_logits(clouds, centers, rid, keep[b // 2:b // 2 + 1].contiguous(), None, num_regions=r, validate=False)
        assert torch.equal(fwd[b // 2:b // 2 + 1], one)


@pytest.mark.parametrize("r", [1, 33, 64])
def test_points_of_a_region_stay_in_ascending_order(r):
    """The logits are maxima and do not see the order of a region's points; the arg-max rows do: of equal values the lower row
    wins, and a row list is the kept regions' points in table order.  128 distinct points, repeated eight times with their
    region ids (copies in every wave's quarter of the cloud): with ascending tables every channel's maximum is attained by a
    first copy.  (The wide entry returns no arg-max rows; its prepare kernel is the same body with larger tables.)"""
    model, _ = probes.coalition_model("pointnet", DEV)
    n, base = 1024, 128
    rng = np.random.default_rng(r)
    pts = np.tile(synth.make_cloud(2, 1024)[0][:base], (n // base, 1))
    rid = np.tile(rng.integers(0, r, size=base), n // base)
    clouds = torch.from_numpy(pts)[None].to(DEV).contiguous()
    centers, ridt = clouds.mean(dim=1).contiguous(), hip_ops.as_i32(rid.reshape(1, n), DEV)
    keep = hip_ops.masks_to_tensor(np.array([(1 << r) - 1], dtype=np.uint64), DEV)
    _, crt = model.engine().coalition_logits(clouds, centers, ridt, keep, None, num_regions=r, return_crt=True)
    assert int(crt.min()) >= 0 and int(crt.max()) < base
