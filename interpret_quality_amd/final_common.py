"""Host-side mirror of the reference's shared Shapley kernel module (tools/final_common.py).

Same function names, argument meaning and return types as the reference, so the stage scripts
read the same; the arithmetic runs in libiq_hip.so.  For PointNet the masked clouds are never
materialised (``model.coalition_logits``); for any other model the masking kernel writes the
batch and the model consumes it, as in the reference.
"""
import time

import numpy as np
import torch

from . import hip_ops, work
from ._lib import IqError


def _is_pointnet(args):
    return args.model == "pointnet" or args.model == "pointnet_roty_da"  # tools/final_common.py:36


def get_reward(logits, lbl, args):
    """tools/final_common.py:11-24.  logits (B',C) -> v (B',)."""
    modified = getattr(args, "softmax_type", "modified") != "normal"  # 'yi'/'minuslog' behave as 'modified'
    return hip_ops.reward(logits.contiguous(), int(lbl[0]), modified)


ALL_CLASSES = "all"     # the ``classes`` argument that names every class of the model


def class_labels(classes, num_classes):
    """``classes`` - ALL_CLASSES or a sequence of labels (any order, repeats allowed) - as a list of ints in [0, num_classes)."""
    c = int(num_classes)
    if isinstance(classes, str):
        if classes != ALL_CLASSES:
            raise IqError("classes must be %r or a sequence of labels, got %r" % (ALL_CLASSES, classes))
        return list(range(c))
    labels = [int(x) for x in np.asarray(classes).reshape(-1)]
    if not labels or any(not 0 <= x < c for x in labels):
        raise IqError("classes must name at least one label in [0, %d), got %r" % (c, labels))
    return labels


def get_reward_classes(logits, classes, args, out=None, first=0):
    """``get_reward`` for the labels ``classes`` (``class_labels``) of the same logits (B',C) -> (G,B'), row g the bits of
    get_reward with lbl = classes[g]; with ``out`` (G,M) written into out[:, first:first+B'] (hip_ops.reward_classes)."""
    modified = getattr(args, "softmax_type", "modified") != "normal"
    return hip_ops.reward_classes(logits.contiguous(), class_labels(classes, logits.shape[1]), modified, out, first)


class RewardSink:
    """Where the rewards of a game's ``columns`` coalitions go, one chunk of logits at a time.  One label ``lbl`` (``classes``
    None): ``v`` is a (columns,) float32 vector, allocated here or the caller's ``out`` view, filled by ``get_reward``.  The
    labels ``classes`` (``class_labels``; ``lbl`` is then not read): ``v`` is the (G,columns) table that ``get_reward_classes``
    fills through its out/first form, row g the bits of the single-label sink with lbl = classes[g]; it exists
    from the first chunk on, since under ALL_CLASSES only the logits say what G is."""

    def __init__(self, lbl, classes, args, columns, device, out=None):
        self.game, self.columns, self.device = (lbl, classes, args), int(columns), device
        self.v = out if out is not None or classes is not None else torch.empty((self.columns,), dtype=torch.float32, device=device)

    def put(self, logits, first):
        """Score ``logits`` (B,C), the logits of coalitions first .. first + B - 1."""
        lbl, classes, args = self.game
        if classes is None:
            self.v[first:first + logits.shape[0]] = get_reward(logits, lbl, args)
            return
        if self.v is None:
            self.v = torch.empty((len(class_labels(classes, logits.shape[1])), self.columns), dtype=torch.float32, device=self.device)
        get_reward_classes(logits, classes, args, self.v, first)


def rewards_with_ends(logits_of, rows, ends, lbl, classes, args, chunk=1 << 16):
    """Rewards of the coalition rows ``rows`` ((M,) narrow or (M,W) wide) with the two rows ``ends`` - the full and the empty
    coalition - appended, so that all come from the same calls: ``logits_of(part)`` gives the logits of at most ``chunk`` rows
    (and counts its work), a RewardSink scores them -> (v (M,) float32 device tensor, v_full, v_empty floats), or with
    ``classes`` (v (G,M), v_full (G,), v_empty (G,) float64 ndarrays).  Nothing depends on ``chunk``."""
    rows = torch.cat([rows, ends])
    chunk = max(1, int(chunk))
    sink = RewardSink(lbl, classes, args, rows.shape[0], rows.device)
    with torch.no_grad():
        for first in range(0, rows.shape[0], chunk):
            sink.put(logits_of(rows[first:first + chunk].contiguous()), first)
    v = sink.v
    if v.dim() == 2:
        tail = v[:, -2:].cpu().numpy().astype(np.float64)
        return v[:, :-2].contiguous(), tail[:, 0].copy(), tail[:, 1].copy()
    tail = v[-2:].cpu().numpy()
    return v[:-2].contiguous(), float(tail[0]), float(tail[1])


def cal_reward(model, data, lbl, args):
    """tools/final_common.py:26-43.  data (B',N,3) -> (v (B',), logits (B',C))."""
    x = data.permute(0, 2, 1).contiguous()
    work.add(x.shape[0])
    out = model(x)
    logits = out[0] if _is_pointnet(args) else out
    return get_reward(logits, lbl, args), logits


def mask_data_batch(masked_data, center, orders, region_id, args):
    """tools/final_common.py:46-61.  In-place on ``masked_data`` ((R+1)*bs, N, 3), which holds
    bs*(R+1) copies of one cloud on entry (tools/final_common.py:88); one launch instead of
    R*bs index assignments."""
    dev = masked_data.device
    cloud = masked_data[-1].clone()  # the last row of a block is never masked
    hip_ops.check_host_indices(np.asarray(orders), 0, args.num_regions, "orders")
    out = hip_ops.mask_shapley(cloud, hip_ops.region_ids(region_id, dev, args.num_regions), hip_ops.as_i32(np.asarray(orders), dev),
                               center.contiguous(), channel_first=False)
    masked_data.copy_(out)
    return masked_data


def prefix_keep_masks(orders, num_regions):
    """(S,R) permutations -> (S*(R+1),) uint64 keep masks: row i of order o keeps orders[o][:i]."""
    hip_ops.check_host_indices(orders, 0, num_regions, "orders")
    return hip_ops.region_words(orders, num_regions, prefixes=True).reshape(-1)


def distinct_coalitions(keep_masks):
    """Prefix coalitions of different permutations coincide as SETS (the empty and the full set once per permutation,
    the 32 single-region sets, ...): of the 3300 coalitions of 100 permutations over 32 regions about 2950 are distinct,
    of 33 000 about 27 700.  Equal sets are equal clouds, hence equal logits (a coalition's logits do not depend on
    what else is in a launch - tested bitwise), so each distinct set is evaluated once and its row is replicated.
    Returns (unique masks, inverse index) with ``unique[inverse] == keep_masks``."""
    k = np.asarray(keep_masks, dtype=np.uint64).reshape(-1)
    if k.size == 0:
        return k, np.zeros((0,), dtype=np.int64)
    # one stable sort + a flag scan (np.unique(..., return_inverse=True) takes 40-180 ms on 33 000 masks here, more than the
    # forward passes it saves; this takes 2 ms)
    idx = np.argsort(k, kind="stable")
    ks = k[idx]
    first = np.empty(k.size, dtype=bool)
    first[0] = True
    first[1:] = ks[1:] != ks[:-1]
    inv = np.empty(k.size, dtype=np.int64)
    inv[idx] = np.cumsum(first) - 1
    return ks[first], inv


def coalition_logits_capped(model, clouds, centers, rid, keep, num_regions, cap):
    """model.coalition_logits on one source cloud, at most ``cap`` coalitions per launch (cap None / 0: one launch)."""
    if not cap or keep.numel() <= cap:
        return model.coalition_logits(clouds, centers, rid, keep, None, num_regions=num_regions, validate=False)
    return torch.cat([model.coalition_logits(clouds, centers, rid, keep[i:i + cap].contiguous(), None, num_regions=num_regions,
                                             validate=False) for i in range(0, keep.numel(), cap)], dim=0)


def dense_logits(model, keep, bs, mask_op):
    """For a model without a coalition entry point: ``mask_op(keep rows, channel_first)`` (the mask kernel, narrow or wide) writes
    the clouds of ``keep`` in batches of ``bs`` and the model consumes them, as in the reference."""
    points_api = hasattr(model, "forward_points")  # consumes (B,N,3) directly: no transpose
    chunks = []
    for i in range(0, keep.shape[0], bs):
        out = mask_op(keep[i:i + bs].contiguous(), not points_api)
        out = model.forward_points(out) if points_api else model(out)
        chunks.append(out[0] if isinstance(out, tuple) else out)
    return torch.cat(chunks, dim=0) if chunks else torch.empty((0, 0), dtype=torch.float32, device=keep.device)


def materialised_logits(model, cloud, rid, keep, center, bs):
    """dense_logits for ``keep`` ((B,) masks of ``cloud`` (N,3))."""
    return dense_logits(model, keep, bs, lambda k, cf: hip_ops.mask_coalitions(cloud, rid, k, center, channel_first=cf))


def masked_logits(model, data, center, rid, keep, args, knob):
    """Logits of the coalitions ``keep`` of one cloud ``data`` (1,N,3).  ``knob``: config.py's batch size in clouds - a floor
    unless strict_batch_cap is set (rows are independent in eval mode, so larger launches give the same logits; stage 1 sets
    no batch size: the reference evaluates one permutation per forward there, final_shapley_value.py:138-144), then a cap."""
    strict = getattr(args, "strict_batch_cap", False)
    if hasattr(model, "coalition_logits"):
        return coalition_logits_capped(model, data.contiguous(), center.reshape(1, 3).contiguous(), rid.reshape(1, -1), keep,
                                       args.num_regions, knob if strict else None)
    bs = knob if strict else max(knob, getattr(model, "preferred_clouds_per_call", 0))
    return materialised_logits(model, data[0].contiguous(), rid, keep, center.reshape(3).contiguous(), bs)


def shapley_logits(model, data, lbl, region_id, orders, args, center=None):
    """Logits of all prefix coalitions of ``orders`` ((S,R) ndarray) for one cloud (1,N,3), in the reference's row order
    (row o*(R+1)+i keeps orders[o][:i]).  Models with a coalition entry point take the region bit masks directly;
    for the others the mask kernel writes the distinct coalitions' clouds in batches of at least
    ``args.shapley_batch_size`` permutations' worth."""
    dev = data.device
    r = args.num_regions
    if center is None:
        center = torch.mean(data, dim=1)  # (1,3), tools/final_common.py:80
    rid = hip_ops.region_ids(region_id, dev, r)   # validated here: the model calls below skip their own check
    uniq, inv = distinct_coalitions(prefix_keep_masks(orders, r))
    work.add(inv.size, uniq.size)
    inv_t = torch.from_numpy(inv.astype(np.int64)).to(dev)
    logits = masked_logits(model, data, center, rid, hip_ops.masks_to_tensor(uniq, dev), args,
                           getattr(args, "shapley_batch_size", 1) * (r + 1))
    return logits.index_select(0, inv_t)


def shap_sampling_all_regions_batch(model, data_disturb, lbl, region_id, load_order_list, args):
    """tools/final_common.py:64-103.  Returns (region_shap_value (R,) float64 ndarray,
    all_logits_this_pose (num_samples*(R+1), C) tensor).  As in the reference only
    ``(num_samples // bs) * bs`` permutations are evaluated while the sum is divided by
    ``num_samples`` (:78,:97); a batch size that does not divide num_samples is rejected up front
    instead of tripping the assert at :99."""
    bs = args.shapley_batch_size
    if args.num_samples % bs != 0:
        raise IqError("shapley_batch_size=%d does not divide num_samples=%d (tools/final_common.py:78,99)"
                      % (bs, args.num_samples))
    t_start = time.time()
    orders = np.asarray(load_order_list[:args.num_samples])
    with torch.no_grad():
        logits = shapley_logits(model, data_disturb, lbl, region_id, orders, args)
        v = get_reward(logits, lbl, args)
        phi_sum, _, _ = hip_ops.shapley_accum(v, hip_ops.as_i32(orders, data_disturb.device))
        region_shap_value = phi_sum.cpu().numpy()  # the only device->host sync of the pose
    region_shap_value /= args.num_samples
    assert logits.size()[0] == args.num_samples * (args.num_regions + 1)
    if getattr(args, "verbose", True):
        print("done time: ", time.time() - t_start)
    return region_shap_value, logits
