"""Exact Shapley values, all-order pairwise interactions and Harsanyi dividends by full enumeration.

Everything else in this package SAMPLES the game, as the reference does (1000 permutations per cloud,
final_shapley_value.py:59-72; at most 100 contexts per pair and order, final_gen_pair.py:25-41).  With n <= 24 players the
coalition engines are fast enough to evaluate all 2^n coalitions: ``value_table`` does that, in chunks, with the masks
enumerated on the device, and the reductions of csrc/iq_lattice.hip turn the table into the quantities the sampled stages
estimate.  A game has n players; player k is region ``players[k]`` (default: region k, n = args.num_regions); coalition index
c has bit k set when player k is present.
"""
import numpy as np
import torch

from . import final_common, hip_ops, work
from ._lib import IqError

MAX_PLAYERS = hip_ops.MAX_EXACT_PLAYERS


def _players(args, players):
    if players is None:
        n = int(args.num_regions)
        if n > MAX_PLAYERS:
            raise IqError("an exact game enumerates 2^n coalitions: n=%d players is above the limit of %d - name at most %d "
                          "regions in players= (the others go into base= or stay masked)" % (n, MAX_PLAYERS, MAX_PLAYERS))
        return None, n
    pl = np.asarray(players, dtype=np.int64).reshape(-1)
    if not 1 <= pl.size <= MAX_PLAYERS:
        raise IqError("players must name 1..%d regions, got %d" % (MAX_PLAYERS, pl.size))
    hip_ops.check_host_indices(pl, 0, int(args.num_regions), "players")
    return pl, int(pl.size)


def value_table(model, data, lbl, region_id, args, players=None, base=0, chunk=1 << 16, classes=None):
    """Rewards of ALL coalitions of one cloud ``data`` (1,N,3): (2^n,) float32 on the device, v[c] = iq_reward of the logits of
    the cloud that keeps ``base`` and the regions players[k] of the set bits k of c (every other point collapses onto the centre,
    the mean of the cloud: tools/final_common.py:80).  ``chunk`` coalitions at a time go through the model's own
    ``coalition_logits`` (which splits launches by the memory that is free), so the logits of 2^24 coalitions are never resident
    at once; a coalition's logits do not depend on what else is in its launch, so the table does not depend on ``chunk``.
    ``classes`` (a sequence of labels, or "all"; ``lbl`` is then not read): the tables of every label from the same logits,
    (G, 2^n), row g the bits of the call with lbl = classes[g]."""
    if not hasattr(model, "coalition_logits"):
        raise IqError("%s has no coalition entry point" % type(model).__name__)
    dev = data.device
    r = int(args.num_regions)
    pl, n = _players(args, players)
    if int(base) >> r:
        raise IqError("base=%#x names a region outside [0, %d)" % (int(base), r))
    chunk = max(1, int(chunk))
    rid = hip_ops.region_ids(region_id, dev, r).reshape(1, -1)
    clouds = data.contiguous()
    centers = torch.mean(data, dim=1).reshape(1, 3).contiguous()
    sink = final_common.RewardSink(lbl, classes, args, 1 << n, dev)
    with torch.no_grad():
        for first in range(0, 1 << n, chunk):
            count = min(chunk, (1 << n) - first)
            keep = hip_ops.enum_keep_masks(first, count, n, dev, pl, base)
            work.add(count)
            sink.put(model.coalition_logits(clouds, centers, rid, keep, None, num_regions=r, validate=False), first)
    return sink.v


def _table(model, data, lbl, region_id, args, players, base, chunk, v):
    return v if v is not None else value_table(model, data, lbl, region_id, args, players, base, chunk)


def shapley(model, data, lbl, region_id, args, players=None, base=0, chunk=1 << 16, v=None):
    """-> (phi (n,) float64 ndarray, v_full, v_empty): the exact Shapley values of the n players and the rewards of the grand and
    the empty coalition (phi sums to their difference).  ``v``: a table ``value_table`` already returned for the same game."""
    v = _table(model, data, lbl, region_id, args, players, base, chunk, v)
    phi = hip_ops.exact_shapley(v).cpu().numpy()
    ends = v[[v.numel() - 1, 0]].cpu().numpy()
    return phi, float(ends[0]), float(ends[1])


def interactions(model, data, lbl, region_id, args, players=None, base=0, chunk=1 << 16, pairs=None, v=None):
    """-> (P, n-1) float64 ndarray: for pair p (player positions; None: all n(n-1)/2 pairs, hip_ops.all_pairs) and order m the
    interaction I_ij^(m) of final_cal_interactions.py:28-36 averaged over ALL contexts of m players."""
    v = _table(model, data, lbl, region_id, args, players, base, chunk, v)
    return hip_ops.exact_interactions(v, pairs).cpu().numpy()


def dividends(model, data, lbl, region_id, args, players=None, base=0, chunk=1 << 16, v=None):
    """-> (2^n,) float64 ndarray of Harsanyi dividends (the Moebius transform of the value table)."""
    v = _table(model, data, lbl, region_id, args, players, base, chunk, v)
    return hip_ops.moebius(v).cpu().numpy()


def sampled_from_table(v, orders, counts):
    """What the sampling stage computes from the permutations ``orders`` ((S,n) of player positions), read off the table
    instead of run through the network (equal coalitions are equal clouds, hence equal rewards): (running sums {count: (n,)},
    per-permutation rows (S,n) float64) as shapley_stage.shapley_all_orders returns them."""
    orders = np.asarray(orders)
    s, n = orders.shape
    if v.numel() != 1 << n:
        raise IqError("orders of %d players against a table of %d coalitions" % (n, v.numel()))
    idx = final_common.prefix_keep_masks(orders, n).astype(np.int64)
    rewards = v.index_select(0, torch.from_numpy(idx).to(v.device)).contiguous()
    return hip_ops.shapley_snapshots(rewards, hip_ops.as_i32(orders, v.device), counts)[:2]


def sampling_error(phi, snaps, rows):
    """Deviation of the running sampled estimate from the exact values ``phi``: per sample count the max and RMS over the
    players, in reward units and in units of the estimate's own standard error (std of the permutation rows / sqrt(count))."""
    out = []
    for count, running in sorted(snaps.items()):
        err = running / count - phi
        se = rows[:count].std(axis=0, ddof=1) / np.sqrt(count) if count > 1 else np.full_like(phi, np.nan)
        z = err / np.where(se > 0, se, np.nan)
        out.append({"samples": int(count), "max_abs_error": float(np.abs(err).max()), "rms_error": float(np.sqrt((err ** 2).mean())),
                    "max_abs_error_in_se": float(np.nanmax(np.abs(z))) if np.isfinite(z).any() else None,
                    "rms_error_in_se": float(np.sqrt(np.nanmean(z ** 2))) if np.isfinite(z).any() else None})
    return out
