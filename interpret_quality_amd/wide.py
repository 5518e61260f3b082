"""Wide games: Shapley values over more than 64 regions, up to one region per point.

Everywhere else in this package a coalition is one uint64 bit mask, so a game has at most 64 regions.  In the reference
NUM_REGIONS is a constant one edits (tools/final_util.py:20-22) and mask_data_batch, cal_region_id and the sampling loop work
for any region count up to the number of points.  Here a WIDE coalition is a row of W = ceil(R / 64) uint64 words - bit
(r & 63) of word (r >> 6) set = region r kept - for 1 <= R <= MAX_REGIONS (include/iq.h, "Wide coalitions").

PointNet evaluates wide coalitions fused (iq_pointnet_coalitions_wide: no masked cloud is ever written).  Every other family
runs iq_mask_coalitions_wide in batches into its own dense forward, the route final_common.materialised_logits takes: correct,
at dense-forward speed.  The interaction, smoothness and pose stages have no wide form.
"""
import numpy as np
import torch

from . import final_common, hip_ops, work
from ._lib import IqError

MAX_REGIONS = hip_ops.MAX_WIDE_REGIONS
DENSE_BATCH = 256     # materialised clouds per dense forward of the families without a wide coalition path


def prefix_keep_masks(orders, num_regions):
    """(S,R) permutations -> (S*(R+1), W) uint64 keep rows on the host: row o*(R+1)+i keeps orders[o][:i]
    (tools/final_common.py:56-60).  An entry outside [0, R) is ignored, as iq_prefix_keep_masks_wide ignores it."""
    r = int(num_regions)
    w = hip_ops.wide_words(r)
    orders = np.asarray(orders, dtype=np.int64)
    if orders.ndim != 2 or orders.shape[1] != r:
        raise IqError("orders must be (S, %d), got %s" % (r, orders.shape))
    s = orders.shape[0]
    valid = (orders >= 0) & (orders < r)
    word = np.where(valid, orders >> 6, -1)
    bit = np.left_shift(np.uint64(1), (orders & 63).astype(np.uint64))
    out = np.zeros((s, r + 1, w), dtype=np.uint64)
    for k in range(w):
        out[:, 1:, k] = np.bitwise_or.accumulate(np.where(word == k, bit, np.uint64(0)), axis=1)
    return out.reshape(s * (r + 1), w)


def _keep_rows(keep, num_regions, device):
    if isinstance(keep, np.ndarray):
        keep = hip_ops.wide_masks_to_tensor(keep, device)
    w = hip_ops.wide_words(num_regions)
    if keep.dim() != 2 or keep.shape[1] != w:
        raise IqError("keep must be (B, %d) for %d regions, got %s" % (w, int(num_regions), tuple(keep.shape)))
    return keep.contiguous()


def coalition_logits(model, data, region_id, keep, args):
    """Logits of the wide coalitions ``keep`` ((B,W) int64-typed device tensor or uint64 ndarray) of one cloud ``data`` (1,N,3);
    every masked point collapses onto the mean of the cloud (tools/final_common.py:80).  ``args``: model, num_regions."""
    r = int(args.num_regions)
    return _logits(model, data, hip_ops.region_ids(region_id, data.device, r), _keep_rows(keep, r, data.device), r)


def _logits(model, data, rid, keep, r):
    """coalition_logits on validated region ids (int32 device tensor) and a (B,W) device tensor."""
    dev = data.device
    center = torch.mean(data, dim=1)
    work.add(keep.shape[0])
    if hasattr(model, "coalition_logits_wide"):
        return model.coalition_logits_wide(data.contiguous(), center.reshape(1, 3).contiguous(), rid.reshape(1, -1), keep, None,
                                           num_regions=r, validate=False)
    points_api = hasattr(model, "forward_points")     # consumes (B,N,3) directly: no transpose
    bs = max(DENSE_BATCH, getattr(model, "preferred_clouds_per_call", 0))
    cloud, c3 = data[0].contiguous(), center.reshape(3).contiguous()
    chunks = []
    for i in range(0, keep.shape[0], bs):
        x = hip_ops.mask_coalitions_wide(cloud, rid, keep[i:i + bs].contiguous(), c3, r, channel_first=not points_api)
        out = model.forward_points(x) if points_api else model(x)
        chunks.append(out[0] if isinstance(out, tuple) else out)
    if not chunks:
        return torch.empty((0, 0), dtype=torch.float32, device=dev)
    return torch.cat(chunks, dim=0)


def shapley(model, data, lbl, region_id, orders, args, snap_counts=None, perms_per_step=None):
    """The sampling loop of final_shapley_value.py:138-156 for one cloud ``data`` (1,N,3) and the permutations ``orders`` ((S,R)
    ndarray): -> (running sums {count: (R,) float64} at ``snap_counts``, per-permutation rows (S,R) float64, total (R,)), shaped
    like shapley_stage.shapley_all_orders.  The prefix masks are built on the device, ``perms_per_step`` permutations at a time
    (default: about 2^17 coalitions), so the keep rows and logits of 1000 x 1025 coalitions are never resident at once.  Prefix
    sets of different permutations almost never coincide at these region counts: no de-duplication."""
    dev = data.device
    r = int(args.num_regions)
    hip_ops.wide_words(r)
    orders = np.asarray(orders)
    if orders.ndim != 2 or orders.shape[1] != r:
        raise IqError("orders must be (S, %d), got %s" % (r, orders.shape))
    hip_ops.check_host_indices(orders, 0, r, "orders")
    s = orders.shape[0]
    step = int(perms_per_step) if perms_per_step else max(1, (1 << 17) // (r + 1))
    orders_dev = hip_ops.as_i32(orders, dev)
    rid = hip_ops.region_ids(region_id, dev, r)
    v = torch.empty((s * (r + 1),), dtype=torch.float32, device=dev)
    with torch.no_grad():
        for lo in range(0, s, step):
            hi = min(lo + step, s)
            keep = hip_ops.prefix_keep_masks_wide(orders_dev[lo:hi].contiguous())
            logits = _logits(model, data, rid, keep, r)
            v[lo * (r + 1):hi * (r + 1)] = final_common.get_reward(logits, lbl, args)
    counts = [int(c) for c in (snap_counts or []) if c <= s]
    total, rows, snaps = hip_ops.shapley_accum_wide(v, orders_dev, snap_counts=counts)
    snaps = snaps.cpu().numpy() if snaps is not None else np.zeros((0, r))
    return {c: snaps[k] for k, c in enumerate(counts)}, rows.cpu().numpy(), total.cpu().numpy()
