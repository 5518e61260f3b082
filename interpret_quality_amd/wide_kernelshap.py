"""The regression (KernelSHAP) estimator of region Shapley values for WIDE games: 65 .. 1024 regions, up to one region per point.

kernelshap.py is the estimator for 2 .. 64 regions (a row is one uint64); this module is its ``gram="analytic"`` variant on wide
keep rows ((M,W) int64-typed, W = ceil(R / 64): wide.py), with the same contract (include/iq.h, "The regression (KernelSHAP)
estimator"):

* sizes: p(s) ~ 1 / (s (R - s)), s = 1 .. R-1, by inverse CDF from ONE ``np.random.random_sample(S)`` on NumPy's global legacy
  generator; members: the first s_m entries of permutation m, the S permutations drawn after the sizes on the device from the same
  stream (``hip_ops.sample_permutations_wide``), a chunk of samples at a time - the full permutations of 512 k samples of 1024
  regions would be 2 GB - each chunk turned into keep rows before the next is drawn; the state is handed back to the host;
* or, ``draw="counter"``, sizes and members by the counter-based contract (``draw_counter``; include/iq.h, "The COUNTER-BASED
  draw"): Philox4x32-10 keyed by (seed, stream), row m a function of (seed, stream, m, R) alone, one launch, no generator state;
* pairing (default): row 2m is S_m, row 2m+1 its complement, M = 2S rows;
* A is the expectation of z z^T under the size law, alpha I + c 1 1^T, so the constrained solve is the closed form
  ``phi_i = 2 H_{R-1} (b_i - mean(b)) + delta / R`` with b = (1/W) sum w z (v - v0): no matrix, no factorisation, no singular case,
  sum(phi) = delta by construction, no running count is ever left out;
* all 2^R - 2 proper coalitions with the weights of ``kernelshap.enumeration_weights`` give the exact Shapley vector (the entry
  points take 2 .. 1024 regions, so ``estimate`` runs the enumerated rows of 2 .. 24 regions too: the identity the tests hold).

The A of SAMPLED rows above 64 regions is not built: ``gram="sampled"`` is an IqError here (``SAMPLED_REFUSAL`` says why).
The moment and phi run in libiq_hip.so (csrc/iq_kshap_wide.hip): float64, ``kshap_accum``'s order, bitwise repeatable.
"""
import sys

import numpy as np
import torch

from . import final_common, hip_ops, kernelshap, wide
from ._lib import IqError

MAX_REGIONS = hip_ops.MAX_WIDE_REGIONS
GRAMS = ("analytic",)
DRAWS = ("stream", "counter")   # the contract the rows are drawn by: NumPy's MT19937 stream (the default), or Philox by (seed, stream, row)
DRAW_CHUNK = 4096      # samples drawn per step of ``draw``: 16 MB of permutations at 1024 regions
SAMPLED_REFUSAL = ("the wide estimator has gram='analytic' only: the sampled Gram matrix of more than 64 regions needs an R x R "
                   "float64 factorisation over several workgroups and more rows than regions before it is regular, and on the one "
                   "game measured it was behind the analytic variant at every budget (kernelshap.estimate has it up to 64 regions)")

regions = hip_ops.kshap_regions_wide
default_samples = kernelshap.default_samples      # 1000 (R + 1), even: no region count enters but through the argument
running_counts = kernelshap.running_counts        # c (R + 1) for c in stage 1's sample counts
pairs = kernelshap.pairs                          # all-pairs interactions: one entry for both row formats, here on (M,W) rows
pairs_se = kernelshap.pairs_se                    # and their standard errors
pairs_cv = kernelshap.pairs_cv                    # and the control-variate estimate (the regression surrogate: 64 regions at most)
CONTROLS = ("none", "shift")                      # what ``game`` offers: a wide game's rows are wide whatever its region count
LIST_CONTROLS = kernelshap.LIST_CONTROLS          # and the sparse surrogate on a pair list, which takes wide rows


def check_gram(gram):
    if gram == "sampled":
        raise IqError(SAMPLED_REFUSAL)
    if gram not in GRAMS:
        raise IqError("gram must be one of %s, got %r" % (GRAMS, gram))


def end_rows(r, device):
    """The full and the empty coalition of R regions: the two rows ``rewards`` appends -> (2,W) int64-typed."""
    rows = np.stack([hip_ops.region_words(np.arange(r), r), np.zeros(hip_ops.wide_words(r), dtype=np.uint64)])
    return hip_ops.wide_masks_to_tensor(rows, device)


def size_cdf(r):
    """(R-1,) float64: entry s-1 = P(size <= s) under p(s) = (1 / (s (R - s))) / Z; the last entry is exactly 1.0."""
    return kernelshap._size_cdf(regions(r))


def draw_sizes(r, count):
    """``count`` coalition sizes by the contract: one random_sample call on NumPy's global generator -> (count,) int32."""
    return kernelshap._draw_sizes(regions(r), count)


def draw(r, samples, paired=True, device="cuda", chunk=DRAW_CHUNK, skip=False):
    """One cloud's draw of ``samples`` rows (paired: rounded down to even, half of them drawn) -> (keep (M,W) int64-typed device
    tensor, sizes (S,) int32 ndarray).  S doubles on the host, then S permutations on the device, ``chunk`` samples at a time, each
    chunk turned into keep rows before the next is drawn; NumPy's global generator is left where a host-only draw would leave it.
    Rows and end state do not depend on ``chunk``.  ``skip``: the same draws, nothing written (keep is None): the draw of a cloud
    that is not selected."""
    r = regions(r)
    s = kernelshap.draws(samples, paired)
    chunk = max(1, int(chunk))
    sizes = draw_sizes(r, s)
    state = hip_ops.mt_state_to_device(device)
    keep = None
    if skip:
        hip_ops.sample_permutations_wide(state, s, r, skip=True)
    else:
        per = 2 if paired else 1
        keep = torch.empty((per * s, hip_ops.wide_words(r)), dtype=torch.int64, device=state.device)
        sizes_dev = torch.from_numpy(sizes).to(state.device)
        for lo in range(0, s, chunk):
            orders = hip_ops.sample_permutations_wide(state, min(chunk, s - lo), r)
            keep[per * lo:per * (lo + chunk)] = hip_ops.kshap_keep_masks_wide(orders, sizes_dev[lo:lo + chunk].contiguous(), paired)
    hip_ops.mt_state_to_host(state, set_global=True)
    return keep, sizes


_draw_stream = draw      # ``game`` and ``shapley`` have an argument of that name


def drawer(kind, seed=1, stream=0):
    """The ``draw`` argument of ``game`` (``kind`` in DRAWS, else IqError) -> the (r, samples, paired, device) -> (keep, sizes) that
    draws a cloud's rows: ``draw``, or ``draw_counter`` keyed by (``seed``, ``stream``)."""
    if kind not in DRAWS:
        raise IqError("draw must be one of %s, got %r" % (DRAWS, kind))
    if kind == "stream":
        return _draw_stream
    return lambda r, samples, paired, device: draw_counter(r, samples, seed, stream, paired, device)


def draw_counter(r, samples, seed, stream=0, paired=True, device="cuda", first=0):
    """One cloud's COUNTER-BASED draw of ``samples`` rows (paired: rounded down to even, half of them drawn) -> (keep (M,W)
    int64-typed device tensor, sizes (S,) int32 ndarray): samples ``first .. first + S - 1`` of the cloud ``stream`` under ``seed``
    (include/iq.h, "The COUNTER-BASED draw"), each a pure function of (seed, stream, index, r).  One launch, no
    chunks, no generator state: NumPy's global generator is not touched and a cloud that is not selected draws nothing."""
    r = regions(r)
    s = kernelshap.draws(samples, paired)
    keep, sizes = hip_ops.kshap_draw_counter(seed, stream, first, s, r, size_cdf(r), paired, device)
    return keep, sizes.cpu().numpy()


def enumerated(r, device):
    """``kernelshap.enumerated`` with the rows widened to (2^R - 2, 1): every proper coalition of at most exact.MAX_PLAYERS regions
    and the weight under which the regression returns the exact Shapley vector."""
    r = regions(r)
    if r > hip_ops.MAX_EXACT_PLAYERS:
        raise IqError("an enumerated game has 2^R rows: R=%d is above the limit of %d" % (r, hip_ops.MAX_EXACT_PLAYERS))
    keep, weights = kernelshap.enumerated(r, device)
    return keep.reshape(-1, 1), weights


def estimate(keep, v, v_empty, v_full, r, weights=None, gram="analytic"):
    """phi of the wide rows ``keep`` (M,W) with rewards ``v`` ((M,) float32 device tensor, or (G,M) for G games on the same rows;
    v_empty, v_full: scalars or (G,)) -> float64 ndarray (R,) or (G,R): the moment kernel, then the closed form."""
    r = regions(r)
    check_gram(gram)
    v2, v0, v1 = kernelshap.games(keep, v, v_empty, v_full)
    b, wsum = hip_ops.kshap_moment_wide(keep, v2, v0, r, weights)
    phi = hip_ops.kshap_phi_analytic(b, wsum, v1 - v0).cpu().numpy()
    return phi[0] if v.dim() == 1 else phi


def phi_se(keep, v, v_empty, v_full, r, paired=True, gram="analytic", weights=None):
    """``estimate`` of SAMPLED wide rows with its standard error -> (phi, se): kernelshap.phi_se on this module."""
    return kernelshap.phi_se(keep, v, v_empty, v_full, r, paired, gram, sys.modules[__name__], weights)


def rewards(model, data, lbl, region_id, args, keep, coalitions=None, chunk=1 << 16, classes=None):
    """Rewards of the wide coalitions ``keep`` (M,W) of one cloud ``data`` (1,N,3), evaluated as ``wide.coalition_logits``
    evaluates them (``coalitions``: "dense" or "compact" for a family other than PointNet), ``chunk`` rows per call, the full and
    the empty coalition as two extra rows of the same calls -> (v (M,) float32 device tensor, v_full, v_empty).  ``classes``
    as in kernelshap.rewards: -> (v (G,M), v_full (G,), v_empty (G,)), row g the bits of the call with lbl = classes[g]."""
    mode = wide._pick_coalitions(coalitions, data)
    r = regions(args.num_regions)
    hip_ops.wide_keep(keep, r)
    rid = hip_ops.region_ids(region_id, data.device, r)
    return final_common.rewards_with_ends(lambda part: wide._logits(model, data, rid, part, r, mode), keep, end_rows(r, data.device),
                                          lbl, classes, args, chunk)


def running_estimates(keep, v, v_empty, v_full, r, counts, gram="analytic"):
    """{count: phi of the first ``count`` rows}, every count: there is no singular case."""
    check_gram(gram)
    return kernelshap.running_estimates(keep, v, v_empty, v_full, r, counts, gram, sys.modules[__name__])


def game(model, data, lbl, region_id, args, samples=None, paired=True, gram="analytic", counts=None, coalitions=None, draw="stream",
         seed=1, stream=0, pairs=False, se=False, control="none", control_pairs=None, centres=None):
    """One cloud's sampled (or, at most exact.MAX_PLAYERS regions, enumerated) game with everything the driver stores: dict of
    keep (M,W), weights (None when sampled), v (M,) float32 rewards, v_full, v_empty, phi (R,) and running {count: phi of the
    first ``count`` rows} (kernelshap.play on this module).  ``draw``: "stream" - ``draw`` on NumPy's global generator - or
    "counter" - ``draw_counter`` keyed by (``seed``, ``stream``), which the other kind ignores.  ``pairs``: also interaction
    (R,R), ``pairs`` of the same rows; ``se``: also phi_se (R,) and, with ``pairs``, interaction_se (R,R); ``control="shift"`` or "sparse" (with ``pairs``; ``control_pairs`` and ``centres`` as kernelshap.play takes them): also interaction_cv, interaction_cv_se and control (``pairs_cv``).  The region count, ``gram`` and ``draw`` are refused, in that order, before anything else
    is looked at."""
    regions(args.num_regions)
    check_gram(gram)
    return kernelshap.play(sys.modules[__name__], model, data, lbl, region_id, args, samples, paired, gram, counts,
                           drawer(draw, seed, stream), pairs=pairs, se=se, control=control, control_pairs=control_pairs,
                           centres=centres, coalitions=coalitions)


def shapley(model, data, lbl, region_id, args, samples=None, paired=True, gram="analytic", counts=None, coalitions=None, draw="stream",
            seed=1, stream=0):
    """-> (phi (R,) float64 ndarray, v_full, v_empty, running {count: (R,) phi of the first ``count`` rows}) of one cloud."""
    g = game(model, data, lbl, region_id, args, samples, paired, gram, counts, coalitions, draw, seed, stream)
    return g["phi"], g["v_full"], g["v_empty"], g["running"]
