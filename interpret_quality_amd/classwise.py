"""All-class region Shapley values from ONE pass over a game's coalitions.

Every estimator of this package spends its time on the coalition forwards.  Each forward returns a (B,C) logit row and the
single-label stages keep one number of it, the reward of the ground-truth label; the other C - 1 games on the same coalitions -
which regions speak for the class the model predicted instead, which pull towards the runner-up - are paid for and dropped.
Here the logits of a game are evaluated once, exactly as the single-label estimator evaluates them, and scored for G labels:

* ``rewards``        - iq_reward_classes: the (G,B) rewards of G labels, optionally into a slice of a (G,M) table;
* ``from_logits``    - the permutation estimator on logits that exist already (fresh ones, or one pose's slice of a stored
                       all_logits.pt): no model is run;
* ``shapley``        - the permutation estimator, narrow (final_common.shapley_logits) and wide (wide.shapley's checks, steps and
                       routes); the (G, S*(R+1)) reward table is filled step by step and reduced by one iq_shapley_accum_games;
* ``kernel_shapley`` - the regression estimator on the rows kernelshap.game / wide_kernelshap.game draw;
* ``exact``          - the enumerated game, iq_exact_shapley per class.

``classes=None`` means every class of the model, otherwise a sequence of labels (any order, repeats allowed); G is their
number.  The design rule, not only a test: the column of label c carries the BITS that today's single-label call gives with
lbl = c.  Out of scope: class-wise pose sweeps and interaction stages, and sharding over ranks.
"""
import numpy as np
import torch

from . import dist as iqdist
from . import exact as exact_game
from . import final_common, hip_ops, kernelshap, wide, wide_kernelshap
from ._lib import IqError

MAX_CLASSES = 64                  # iq_reward_classes: 2 <= C <= 64, 1 <= G <= 64
MAX_TABLE_FLOATS = 1 << 28        # ``exact``: G * 2^n floats at most (1 GiB of value tables)
NARROW_REGIONS = kernelshap.MAX_REGIONS      # up to here a coalition is one uint64 and the narrow estimators run


def _classes(classes):
    """The ``classes`` argument of this module -> what final_common.class_labels takes (None = every class)."""
    if classes is None:
        return final_common.ALL_CLASSES
    if isinstance(classes, str):
        raise IqError("classes must be None (every class) or a sequence of labels, got %r" % (classes,))
    labels = [int(c) for c in np.asarray(classes).reshape(-1)]
    if not 1 <= len(labels) <= MAX_CLASSES or min(labels) < 0:
        raise IqError("classes must name 1 .. %d labels >= 0, got %r" % (MAX_CLASSES, labels))
    return labels


def num_games(model, classes):
    """G before any forward has run: the labels named, or the class count of the model's logits."""
    cls = _classes(classes)
    return iqdist.num_classes_of(model) if isinstance(cls, str) else len(cls)


def rewards(logits, classes, args, out=None, first=0):
    """logits (B,C) -> (G,B) float32, row g = final_common.get_reward(logits, [classes[g]], args) bit for bit
    (``args.softmax_type`` read as get_reward reads it); with ``out`` (G,M) written into out[:, first:first+B], the rest of
    ``out`` untouched."""
    return final_common.get_reward_classes(logits, _classes(classes), args, out, first)


def _orders(orders, r):
    orders = np.asarray(orders)
    if orders.ndim != 2 or orders.shape[1] != r:
        raise IqError("orders must be (S, %d), got %s" % (r, orders.shape))
    if orders.shape[0] < 1:
        raise IqError("orders holds no permutation")
    return orders


def _reduce(table, orders, snap_counts, se=False):
    """One iq_shapley_accum_games over the (G, S*(R+1)) reward table -> (snaps {count: (G,R)}, total (G,R)), float64 ndarrays;
    ``se``: also the (G,R) standard error of total / S, from one iq_shapley_sq_accum_games over the same table (S >= 2)."""
    counts = [int(c) for c in (snap_counts or []) if c <= orders.shape[0]]
    if se and orders.shape[0] < 2:
        raise IqError("a standard error needs at least 2 permutations, got %d" % orders.shape[0])
    total, snaps = hip_ops.shapley_accum_games(table, orders, counts)
    snaps = snaps.cpu().numpy() if snaps is not None else None
    out = {c: snaps[:, k] for k, c in enumerate(counts)}, total.cpu().numpy()
    if se:
        out += (hip_ops.shapley_se(out[1], hip_ops.shapley_sq_accum_games(table, orders)[0], orders.shape[0]),)
    return out


def from_logits(logits, orders, args, classes=None, snap_counts=None, se=False):
    """The permutation estimator on the logits (S*(R+1), C) of the prefix coalitions of ``orders`` ((S,R) ndarray), in the
    reference's row order (row o*(R+1)+i keeps orders[o][:i]) -> (running sums {count: (G,R)} at the ``snap_counts`` that do not
    exceed S, total (G,R)), float64, not divided; ``se``: and the (G,R) standard error of total / S.  No model is run: fresh
    logits, or one pose's slice of a stored all_logits.pt."""
    r = int(args.num_regions)
    orders = _orders(orders, r)
    if logits.dim() != 2 or logits.shape[0] != orders.shape[0] * (r + 1):
        raise IqError("logits must be (%d, C) for %d permutations of %d regions, got %s"
                      % (orders.shape[0] * (r + 1), orders.shape[0], r, tuple(logits.shape)))
    return _reduce(rewards(logits, classes, args), orders, snap_counts, se)


def shapley(model, data, region_id, orders, args, classes=None, snap_counts=None, route=None, coalitions=None, se=False):
    """The permutation estimator of one cloud ``data`` (1,N,3) for G labels on ONE evaluation of the prefix coalitions of
    ``orders`` ((S,R) ndarray) -> (running sums {count: (G,R)}, total (G,R)), float64, not divided: row g is the total (and the
    running sums) of shapley_stage.shapley_all_orders (up to 64 regions) or wide.shapley (above) with lbl = classes[g], bit for
    bit.  Up to 64 regions the logits are final_common.shapley_logits's; above, wide.shapley's checks, steps and routes run
    (``route``, ``coalitions``: as there; up to 64 regions they are not taken) and the (G, S*(R+1)) reward table is filled step
    by step.  One iq_shapley_accum_games reduces it: no per-class row table.  ``se``: a third value, the (G,R) standard error of
    total / S - the permutations are iid, so it is the column standard error of the per-permutation differences, from their sum of
    squares (iq_shapley_sq_accum_games) and no further forward."""
    cls = _classes(classes)
    r = int(args.num_regions)
    if r <= NARROW_REGIONS:
        if route is not None or coalitions is not None:
            raise IqError("route and coalitions belong to games of more than %d regions" % NARROW_REGIONS)
        orders = _orders(orders, r)
        with torch.no_grad():
            logits = final_common.shapley_logits(model, data, None, region_id, orders, args)
            table = final_common.get_reward_classes(logits, cls, args)
        return _reduce(table, orders, snap_counts, se)
    route, mode, r, orders = wide._game(model, data, orders, args, route, coalitions)
    orders = _orders(orders, r)
    dev = data.device
    orders_dev = hip_ops.as_i32(orders, dev)
    rid = hip_ops.region_ids(region_id, dev, r)
    steps = wide._steps(orders_dev, r)
    keep = None if route == "prefix" else lambda j: hip_ops.prefix_keep_masks_wide(steps[j][2])
    sink = final_common.RewardSink(None, cls, args, orders.shape[0] * (r + 1), dev)
    with torch.no_grad():
        wide._rewards(model, data, rid, steps, keep, sink, r, mode)
    return _reduce(sink.v, orders, snap_counts, se)


def ends(model, data, region_id, args, classes=None, coalitions=None):
    """The two coalitions every permutation shares -> (v_full (G,), v_empty (G,) float64 ndarrays, the full cloud's logits (C,)
    ndarray): one launch of two rows, evaluated as the game's coalitions are (masked_logits up to 64 regions, wide._logits
    above)."""
    cls = _classes(classes)
    r = int(args.num_regions)
    dev = data.device
    rid = hip_ops.region_ids(region_id, dev, r)
    with torch.no_grad():
        if r <= NARROW_REGIONS:
            logits = final_common.masked_logits(model, data, torch.mean(data, dim=1), rid, kernelshap.end_rows(r, dev), args, 2)
        else:
            logits = wide._logits(model, data, rid, wide_kernelshap.end_rows(r, dev), r, wide._pick_coalitions(coalitions, data))
        v = final_common.get_reward_classes(logits, cls, args).cpu().numpy().astype(np.float64)
    return v[:, 0].copy(), v[:, 1].copy(), logits[0].cpu().numpy()


def kernel_shapley(model, data, region_id, args, classes=None, samples=None, paired=True, gram=None, draw="stream", seed=0, stream=0,
                   coalitions=None, se=False):
    """The regression estimator of one cloud for G labels on ONE evaluation of the drawn rows -> (phi (G,R) float64, v_full (G,),
    v_empty (G,)).  The rows are drawn exactly as kernelshap.game (2 .. 64 regions; ``draw`` must be "stream", ``coalitions``
    None) or wide_kernelshap.game (65 .. 1024) draws them, the rewards of the G labels go into a (G,M) table and ``estimate``
    takes it whole: row g is ``kernelshap.shapley`` / ``wide_kernelshap.shapley`` with lbl = classes[g], bit for bit.  ``gram``:
    None = "sampled" up to 64 regions, "analytic" above.  ``samples``: a count, None (default_samples) or "all".  ``se``: a
    fourth value, the (G,R) standard error of phi (the analytic Gram matrix and drawn rows only: ``kernelshap.play``)."""
    cls = _classes(classes)
    narrow = int(args.num_regions) <= NARROW_REGIONS
    ks = kernelshap if narrow else wide_kernelshap
    ks.regions(args.num_regions)
    gram = gram or ("sampled" if narrow else "analytic")
    ks.check_gram(gram)
    if narrow and (draw != "stream" or coalitions is not None):
        raise IqError("draw=%r / coalitions=%r belong to games of more than %d regions" % (draw, coalitions, NARROW_REGIONS))
    how = {} if narrow else {"draw": wide_kernelshap.drawer(draw, seed, stream), "coalitions": coalitions}
    g = kernelshap.play(ks, model, data, None, region_id, args, samples, paired, gram, (), classes=cls, se=se, **how)
    return (g["phi"], g["v_full"], g["v_empty"]) + ((g["phi_se"],) if se else ())


def exact(model, data, region_id, args, classes=None, players=None, base=0):
    """The enumerated game of one cloud for G labels on ONE evaluation of all 2^n coalitions -> (phi (G,n) float64 ndarray,
    tables (G, 2^n) float32 device tensor): row g is exact.shapley / exact.value_table with lbl = classes[g], bit for bit
    (iq_exact_shapley runs per class).  IqError before any launch when G * 2^n exceeds MAX_TABLE_FLOATS floats."""
    cls = _classes(classes)
    _, n = exact_game._players(args, players)
    g = num_games(model, classes)
    if g << n > MAX_TABLE_FLOATS:
        raise IqError("%d classes of 2^%d coalitions are %d floats of value tables, above the limit of 2^28: name fewer classes "
                      "or fewer players" % (g, n, g << n))
    tables = exact_game.value_table(model, data, None, region_id, args, players, base, classes=cls)
    phi = np.stack([hip_ops.exact_shapley(tables[k]).cpu().numpy() for k in range(tables.shape[0])])
    return phi, tables
