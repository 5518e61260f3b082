"""Wide games: Shapley values and multi-order interactions over more than 64 regions, up to one region per point.

Everywhere else in this package a coalition is one uint64 bit mask, so a game has at most 64 regions.  In the reference
NUM_REGIONS is a constant one edits (tools/final_util.py:20-22) and mask_data_batch, cal_region_id and the sampling loop work
for any region count up to the number of points.  Here a WIDE coalition is a row of W = ceil(R / 64) uint64 words - bit
(r & 63) of word (r >> 6) set = region r kept - for 1 <= R <= MAX_REGIONS (include/iq.h, "Wide coalitions").

PointNet evaluates wide coalitions fused (iq_pointnet_coalitions_wide: no masked cloud is ever written), and the prefix
coalitions of permutations - all that the sampled Shapley values need - straight from the permutations
(iq_pointnet_prefix_coalitions_wide, ``prefix_logits``: no keep rows either, the same bits).  Every other family has two ways,
named by the ``coalitions`` argument of the functions below: "dense" (the default, and what None means) runs
iq_mask_coalitions_wide in batches into the family's dense forward (final_common.dense_logits, the narrow route too) - correct,
at dense-forward speed; "compact" takes the family's compact coalition path through its wide entry (``coalition_logits_wide``:
a coalition's distinct rows only, per-source-cloud tables), whose logits agree with the dense forward's to rounding, bitwise only
where the summation order is the same.  For PointNet both names mean its fused path.  Both halves of the project have a wide form: the sampled Shapley values (``shapley``, wide_stage.py)
and the multi-order interactions of sampled (pair, context) coalitions (``gen_context``, ``interaction_logits``, ``interactions``,
wide_interaction_stage.py), and so do the stages that move the cloud: the pose sweeps (``shapley_over_poses`` - ``shapley``'s checks,
launches and reward loop run per pose: ``_game``, ``_steps``, ``_rewards`` - and ``sharded_shapley``,
wide_pose_stage.py) and the smoothness enumeration (smoothness.enumerate_smoothness with ``wide=True``, wide_smoothness_stage.py;
clouds of at most 1024 points).  The random draws - permutations and sampled contexts - come from NumPy's global generator on
the host or, the same stream, from the device sampler (``gen_context`` / ``iter_contexts`` with ``device``, ``skip_contexts``;
hip_ops.sample_permutations_wide).  Not wide: the single-region folders of final_gen_pair.py.
"""
import numpy as np
import torch

from . import dist as iqdist
from . import final_common, gen_pair, hip_ops, interaction, pose_sweep, work
from ._lib import IqError

MAX_REGIONS = hip_ops.MAX_WIDE_REGIONS
DENSE_BATCH = 256     # materialised clouds per dense forward of the families without a wide coalition path
ROUTES = ("prefix", "keep")   # how ``shapley`` evaluates prefix coalitions: from the permutations, or through keep rows
DEFAULT_ROUTE = "prefix"      # what route=None means for a model with ``prefix_logits_wide`` (the measured rule)
COALITIONS = ("dense", "compact")   # how a family other than PointNet evaluates wide coalitions; None = "dense"


def _pick_coalitions(coalitions, data):
    """``coalitions`` -> "dense" or "compact"; "compact" has no CPU form."""
    if coalitions is not None and coalitions not in COALITIONS:
        raise IqError("coalitions must be one of %s or None, got %r" % (COALITIONS, coalitions))
    if coalitions == "compact" and not data.is_cuda:
        raise IqError("coalitions='compact' needs the cloud on a GPU (no CPU fallback)")
    return coalitions or "dense"


def prefix_keep_masks(orders, num_regions):
    """(S,R) permutations -> (S*(R+1), W) uint64 keep rows on the host: row o*(R+1)+i keeps orders[o][:i]
    (tools/final_common.py:56-60).  An entry outside [0, R) is ignored, as iq_prefix_keep_masks_wide ignores it."""
    r = int(num_regions)
    w = hip_ops.wide_words(r)
    orders = np.asarray(orders, dtype=np.int64)
    if orders.ndim != 2 or orders.shape[1] != r:
        raise IqError("orders must be (S, %d), got %s" % (r, orders.shape))
    return hip_ops.region_words(orders, r, prefixes=True).reshape(-1, w)


def coalition_logits(model, data, region_id, keep, args, coalitions=None):
    """Logits of the wide coalitions ``keep`` ((B,W) int64-typed device tensor or uint64 ndarray) of one cloud ``data`` (1,N,3);
    every masked point collapses onto the mean of the cloud (tools/final_common.py:80).  ``args``: model, num_regions.
    ``coalitions``: None / "dense" - a family other than PointNet runs its dense forward on materialised clouds - or "compact" -
    its compact coalition path (IqError for a cloud that path does not take: PointNet++ and PointConv above 1024 points)."""
    mode = _pick_coalitions(coalitions, data)
    r = int(args.num_regions)
    keep = (hip_ops.wide_masks_to_tensor(keep, data.device) if isinstance(keep, np.ndarray) else keep).contiguous()
    hip_ops.wide_keep(keep, r)
    return _logits(model, data, hip_ops.region_ids(region_id, data.device, r), keep, r, mode)


def _fused(model):
    """PointNet: one fused wide path, whatever ``coalitions`` says."""
    return hasattr(model, "prefix_logits_wide")


def _logits(model, data, rid, keep, r, mode="dense"):
    """coalition_logits on validated region ids (int32 device tensor) and a (B,W) device tensor; ``mode`` "dense" or "compact"."""
    center = torch.mean(data, dim=1)
    work.add(keep.shape[0])
    if mode == "compact" or _fused(model):
        return model.coalition_logits_wide(data.contiguous(), center.reshape(1, 3).contiguous(), rid.reshape(1, -1), keep, None,
                                           num_regions=r, validate=False)
    cloud, c3 = data[0].contiguous(), center.reshape(3).contiguous()
    return final_common.dense_logits(model, keep, max(DENSE_BATCH, getattr(model, "preferred_clouds_per_call", 0)),
                                     lambda k, cf: hip_ops.mask_coalitions_wide(cloud, rid, k, c3, r, channel_first=cf))


def _pick_route(model, route):
    """``route`` of ``shapley`` -> "prefix" or "keep"; None = DEFAULT_ROUTE where the model has the prefix entry, else "keep"."""
    if route is not None and route not in ROUTES:
        raise IqError("route must be one of %s or None, got %r" % (ROUTES, route))
    fused = hasattr(model, "prefix_logits_wide")
    if route == "prefix" and not fused:
        raise IqError("route='prefix' needs a model with prefix_logits_wide (PointNet); %s has none" % type(model).__name__)
    return route or (DEFAULT_ROUTE if fused else "keep")


def _prefix_logits(model, data, rid, orders_dev, r, mode="dense"):
    """prefix_logits on validated region ids and an (S,R) int32 device tensor of permutations."""
    if not hasattr(model, "prefix_logits_wide"):
        return _logits(model, data, rid, hip_ops.prefix_keep_masks_wide(orders_dev), r, mode)
    center = torch.mean(data, dim=1)
    work.add(orders_dev.shape[0] * (r + 1))
    return model.prefix_logits_wide(data.contiguous(), center.reshape(1, 3).contiguous(), rid.reshape(1, -1), orders_dev, None,
                                    num_regions=r, validate=False)


def prefix_logits(model, data, region_id, orders, args, coalitions=None):
    """Logits of the prefix coalitions of the permutations ``orders`` ((S,R) ndarray or int32 device tensor) of one cloud ``data``
    (1,N,3): row o*(R+1)+i keeps orders[o][:i] (tools/final_common.py:56-60) - ``coalition_logits`` on
    hip_ops.prefix_keep_masks_wide(orders), bit for bit.  PointNet evaluates them straight from the permutations; a family
    without ``prefix_logits_wide`` goes through the keep rows, evaluated as ``coalitions`` says (``coalition_logits``).
    ``args``: model, num_regions."""
    mode = _pick_coalitions(coalitions, data)
    r = int(args.num_regions)
    hip_ops.wide_words(r)
    if isinstance(orders, np.ndarray):
        orders = hip_ops.as_i32(orders, data.device)
    if orders.dim() != 2 or orders.shape[1] != r:
        raise IqError("orders must be (S, %d), got %s" % (r, tuple(orders.shape)))
    return _prefix_logits(model, data, hip_ops.region_ids(region_id, data.device, r), orders.contiguous(), r, mode)


def _game(model, clouds, orders, args, route, coalitions):
    """What ``shapley`` and ``shapley_over_poses`` check before anything reaches a device -> (route, mode, R, ``orders`` as an (S,R)
    ndarray); the route first, before any other argument is touched."""
    route = _pick_route(model, route)
    mode = _pick_coalitions(coalitions, clouds)
    r = int(args.num_regions)
    hip_ops.wide_words(r)
    orders = np.asarray(orders)
    if orders.ndim != 2 or orders.shape[1] != r:
        raise IqError("orders must be (S, %d), got %s" % (r, orders.shape))
    hip_ops.check_host_indices(orders, 0, r, "orders")
    return route, mode, r, orders


def _steps(orders_dev, r, perms_per_step=None):
    """The launches of a game: [(lo, hi, orders_dev[lo:hi])], ``perms_per_step`` permutations at a time (default: about 2^17
    coalitions)."""
    s = orders_dev.shape[0]
    step = int(perms_per_step) if perms_per_step else max(1, (1 << 17) // (r + 1))
    return [(lo, min(lo + step, s), orders_dev[lo:lo + step].contiguous()) for lo in range(0, s, step)]


def _rewards(model, data, rid, steps, keep, sink, r, mode):
    """The rewards of the S*(R+1) prefix coalitions of one cloud ``data`` (1,N,3) into ``sink`` (a final_common.RewardSink), one
    step of ``_steps`` at a time.  ``keep``: None on the prefix route - a step is evaluated straight from its permutations - else
    step index -> the step's keep rows, evaluated as arbitrary coalitions."""
    for j, (lo, _, step_orders) in enumerate(steps):
        if keep is None:
            logits = _prefix_logits(model, data, rid, step_orders, r, mode)
        else:
            logits = _logits(model, data, rid, keep(j), r, mode)
        sink.put(logits, lo * (r + 1))


def shapley(model, data, lbl, region_id, orders, args, snap_counts=None, perms_per_step=None, route=None, coalitions=None):
    """The sampling loop of final_shapley_value.py:138-156 for one cloud ``data`` (1,N,3) and the permutations ``orders`` ((S,R)
    ndarray): -> (running sums {count: (R,) float64} at ``snap_counts``, per-permutation rows (S,R) float64, total (R,)), shaped
    like shapley_stage.shapley_all_orders.  ``perms_per_step`` permutations at a time (default: about 2^17 coalitions), so the
    logits of 1000 x 1025 coalitions are never resident at once.  ``route``: "prefix" evaluates a step straight from its
    permutations (``prefix_logits``; IqError for a model without that entry), "keep" builds the prefix masks on the device and
    evaluates them as arbitrary coalitions, None takes "prefix" where the model has it - the values are the same bits either
    way.  ``coalitions``: how a family other than PointNet evaluates the keep rows (``coalition_logits``).  Prefix sets of
    different permutations almost never coincide at these region counts: no de-duplication."""
    route, mode, r, orders = _game(model, data, orders, args, route, coalitions)
    dev = data.device
    orders_dev = hip_ops.as_i32(orders, dev)
    rid = hip_ops.region_ids(region_id, dev, r)
    steps = _steps(orders_dev, r, perms_per_step)
    # the keep rows of one step at a time: at R = 1024 and 1000 permutations all of them would be about 130 MB
    keep = None if route == "prefix" else lambda j: hip_ops.prefix_keep_masks_wide(steps[j][2])
    sink = final_common.RewardSink(lbl, None, args, orders.shape[0] * (r + 1), dev)
    with torch.no_grad():
        _rewards(model, data, rid, steps, keep, sink, r, mode)
    return hip_ops.shapley_snapshots(sink.v, orders_dev, snap_counts, hip_ops.shapley_accum_wide)


def shapley_over_poses(model, poses, lbl, region_id, orders, args, route=None, coalitions=None):
    """Region Shapley values of several perturbed copies ``poses`` (P,N,3) of one cloud under the permutations ``orders`` ((S,R)
    ndarray): -> phi (P,R) float64 device tensor, the wide twin of pose_sweep.shapley_over_poses without its logits.  phi[p] is
    ``total / S`` of ``shapley(model, poses[p:p+1], lbl, region_id, orders, args, route=route, coalitions=coalitions)``, bit for bit:
    ``shapley``'s checks, launches and reward loop (``_game``, ``_steps``, ``_rewards``) run per pose, then ``shapley_accum_wide``.
    What does not depend on the pose is done once per call: the checks, the permutations and region ids on the device and, on the
    keep route, the keep rows.  The centre of a pose is torch.mean of that one (1,N,3) cloud, never of a batch of poses
    (pose_sweep.shapley_over_poses records what a batched mean did to sharding).  Every route goes pose by pose: poses do not share
    launches (DESIGN.md 5e has the rule and why).
    ``route`` and ``coalitions`` as in ``shapley``."""
    route, mode, r, orders = _game(model, poses, orders, args, route, coalitions)
    if poses.dim() != 3 or poses.shape[2] != 3:
        raise IqError("poses must be (P, N, 3), got %s" % (tuple(poses.shape),))
    dev = poses.device
    s, p = orders.shape[0], poses.shape[0]
    phi = torch.zeros((p, r), dtype=torch.float64, device=dev)
    if p == 0:          # an empty shard still agrees with the others on the trailing shape of the gather
        return phi
    if s == 0:
        raise IqError("orders holds no permutation")
    per = s * (r + 1)
    orders_dev = hip_ops.as_i32(orders, dev)
    rid = hip_ops.region_ids(region_id, dev, r)
    poses = poses.contiguous()
    with torch.no_grad():
        steps = _steps(orders_dev, r)                 # ``shapley``'s launches
        rows = [hip_ops.prefix_keep_masks_wide(o) for _, _, o in steps] if route == "keep" else None   # once per call, not per pose
        keep = None if rows is None else rows.__getitem__
        v = torch.empty((p * per,), dtype=torch.float32, device=dev)
        for k in range(p):
            sink = final_common.RewardSink(lbl, None, args, per, dev, out=v[k * per:(k + 1) * per])      # a view: no copy
            _rewards(model, poses[k:k + 1], rid, steps, keep, sink, r, mode)
        for k in range(p):
            total, _, _ = hip_ops.shapley_accum_wide(v[k * per:(k + 1) * per], orders_dev)
            # a true float64 division, as ``total / S`` on the host: a tensor divided by a Python number is multiplied by its
            # reciprocal on the device, one rounding more (the values differ in the last bit for S = 3)
            phi[k] = torch.div(total, torch.full_like(total, float(s)))
    return phi


def sharded_shapley(model, data, poses, lbl, region_id, orders, args, route=None, coalitions=None):
    """The wide twin of pose_sweep.sharded_shapley, on its helper (pose_sweep.sharded_over_poses: the original travels as pose 0)
    -> (orig (R,) float64 ndarray, phi (P,R) float64 tensor), the same on every rank whatever the rank count.  One
    all_gather_rows of phi per call; no logits, no other collective."""
    phi, = pose_sweep.sharded_over_poses(data, poses, lambda clouds: (
        shapley_over_poses(model, clouds, lbl, region_id, orders, args, route=route, coalitions=coalitions),))
    return phi[0].cpu().numpy(), phi[1:]


# ---- multi-order interactions: final_gen_pair.py, final_point_binary_interaction_logits.py and final_cal_interactions.py ---------

gen_pair_random = gen_pair.gen_pair_random            # final_gen_pair.py:288-300 does not depend on the region count
interactions = interaction.compute_order_interaction  # final_cal_interactions.py:14-37: reward and reduction never see a mask


_DEVICE_DTYPES = {np.dtype(np.int16): torch.int16, np.dtype(np.int32): torch.int32, np.dtype(np.int64): torch.int64}


def _device_draw(num_regions, cmax, dtype, skip=False):
    """The ``draw`` of gen_pair.iter_contexts_device for a wide game: the heads of P * cmax permutations of R - 2
    (hip_ops.sample_permutations_wide, head = m), mapped to regions on the device (hip_ops.context_regions_wide) and brought to
    the host in ``dtype``; ``skip``: the draw only advances the generator."""
    r = int(num_regions)

    def draw(state, pairs, m):
        p = pairs.shape[0]
        heads = hip_ops.sample_permutations_wide(state, p * cmax, r - 2, head=m, skip=skip)
        if skip:
            return None
        ctx = hip_ops.context_regions_wide(pairs, heads.reshape(p, cmax, m), r)
        on_device = _DEVICE_DTYPES.get(np.dtype(dtype))
        return (ctx if on_device is None else ctx.to(on_device)).cpu().numpy().astype(dtype, copy=False)
    return draw


def iter_contexts(pairs, num_regions, ratios, num_save_context_max, dtype=np.int64, device=None):
    """``gen_context`` one ratio at a time: a generator of (P, C, m) arrays of ``dtype`` (at R = 1024 one ratio's contexts are up
    to 30 000 x 1022 entries: a caller that saves them need not hold thirteen of them).  The draws are gen_pair.iter_contexts's,
    the host loop of the narrow stage - or, with ``device`` (a GPU), the same draws from the device sampler
    (gen_pair.iter_contexts_device: the loop of the narrow stage's device route), host arrays all the same."""
    hip_ops.wide_words(num_regions)
    if device is not None and len(pairs) > 0:
        hip_ops.check_host_indices(np.asarray(pairs), 0, int(num_regions), "pairs")
        yield from gen_pair.iter_contexts_device(pairs, num_regions, ratios, num_save_context_max, device,
                                                 _device_draw(num_regions, int(num_save_context_max), dtype), dtype)
    else:
        yield from gen_pair.iter_contexts(pairs, num_regions, ratios, num_save_context_max, dtype)


def skip_contexts(num_pairs, num_regions, ratios, num_save_context_max, device):
    """Advance NumPy's GLOBAL generator past the contexts of one cloud with ``num_pairs`` pairs, as ``gen_context`` would leave it,
    on the device and without writing anything (iq_sample_permutations_wide's skip mode): the contexts of a cloud that is not
    selected.  How many words a draw consumes does not depend on the pairs."""
    hip_ops.wide_words(num_regions)
    pairs = np.zeros((int(num_pairs), 2), dtype=np.int64)
    draw = _device_draw(num_regions, int(num_save_context_max), np.int64, skip=True)
    if int(num_pairs) > 0:
        for _ in gen_pair.iter_contexts_device(pairs, num_regions, ratios, num_save_context_max, device, draw, skip=True):
            pass


def gen_context(pairs, num_regions, ratios, num_save_context_max, device=None):
    """final_gen_pair.py:18-43 for any region count: for each ratio (in order) the (P, C, m) int64 contexts of the (P,2) ``pairs``,
    m = int((R-2)*ratio) regions out of the R-2 that are not in the pair - ``num_save_context_max`` sampled ones per pair when
    C(R-2, m) exceeds that number, otherwise all combinations.  The draws come from NumPy's GLOBAL generator in the
    reference's order (ratio, pair, context), each as rest[np.random.permutation(R-2)[:m]] - what the reference's
    np.random.choice(rest, m, replace=False) does on the legacy generator, without its per-call overhead: 390 000 draws at
    R = 1024 take seconds on the host.  With ``device`` (a GPU) the generator is continued there for the sampled ratios
    (iq_sample_permutations_wide: the narrow stage's sampler for up to MAX_REGIONS regions) and handed back: the same arrays, and
    the same generator state afterwards."""
    return list(iter_contexts(pairs, num_regions, ratios, num_save_context_max, device=device))


def _pairs_contexts(pairs, contexts, r):
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    ctx = np.asarray(contexts)
    if ctx.ndim != 3 or ctx.shape[0] != pairs.shape[0] or ctx.shape[2] > r:
        raise IqError("contexts must be (%d, C, m <= %d), got %s" % (pairs.shape[0], r, ctx.shape))
    return pairs, ctx


def context_keep_masks(pairs, contexts, num_regions):
    """(P,2) pairs and (P,C,m) contexts -> (4*P*C, W) uint64 keep rows on the host, rows 4k .. 4k+3 = S+{i,j}, S+{i}, S+{j}, S
    (final_point_binary_interaction_logits.py:45-52).  A pair or context entry outside [0, R) is ignored, as
    iq_context_keep_masks_wide ignores it; for R <= 64 the words are interaction.context_keep_masks's."""
    r = int(num_regions)
    w = hip_ops.wide_words(r)
    pairs, ctx = _pairs_contexts(pairs, contexts, r)
    p, c = ctx.shape[0], ctx.shape[1]
    s = hip_ops.region_words(ctx, r)                      # (P,C,W)
    bi, bj = hip_ops.region_words(pairs[:, None, :1], r), hip_ops.region_words(pairs[:, None, 1:], r)
    return np.stack([s | bi | bj, s | bi, s | bj, s], axis=2).reshape(4 * p * c, w)


def interaction_logits(model, data, region_id, pairs, contexts, args, coalitions=None):
    """final_point_binary_interaction_logits.py:15-70 for a wide game: the logits of the four coalitions S+{i,j}, S+{i}, S+{j}, S
    of every (pair, context) of ONE ratio on one cloud ``data`` (1,N,3), perturbed or not (masked points collapse onto
    torch.mean(data, dim=1)) -> (P, 4C, K) float32.  ``pairs`` (P,2), ``contexts`` (P,C,m) host arrays of any integer type;
    ``args``: model, num_regions.  The contexts go to the device as int32 (at most about 110 MB at R = 1024), the keep rows are
    built there (iq_context_keep_masks_wide) and evaluated as ``coalition_logits`` evaluates them: PointNet fused, in launches of
    at most 2^16 coalitions, every other family through its dense forward or, with ``coalitions="compact"``, its compact
    path.  Sampled contexts of more than 64 regions do not
    coincide: no de-duplication (interaction.compute_order_interaction_logits, the narrow stage, evaluates distinct sets once)."""
    mode = _pick_coalitions(coalitions, data)
    dev = data.device
    r = int(args.num_regions)
    hip_ops.wide_words(r)
    pairs, ctx = _pairs_contexts(pairs, contexts, r)
    hip_ops.check_host_indices(pairs, 0, r, "pairs")
    hip_ops.check_host_indices(ctx, 0, r, "contexts")
    p, c = ctx.shape[0], ctx.shape[1]
    if p * c == 0:
        return torch.zeros((p, 4 * c, iqdist.num_classes_of(model)), dtype=torch.float32, device=dev)
    rid = hip_ops.region_ids(region_id, dev, r)
    with torch.no_grad():
        keep = hip_ops.context_keep_masks_wide(hip_ops.as_i32(pairs, dev), hip_ops.as_i32(ctx, dev), r)
        logits = _logits(model, data, rid, keep, r, mode)
    return logits.reshape(p, 4 * c, -1)
