"""The regression (KernelSHAP) estimator of region Shapley values, for games of 2 .. 64 regions.

Stage 1 (shapley_stage.py) estimates Shapley values as the reference does, by walking sampled permutations.  This module is the
weighted least-squares estimator with paired sampling on the same coalition engines: sample coalitions from the Shapley kernel,
regress their rewards on their membership rows under the constraint sum(phi) = v(all) - v(empty).  The contract (include/iq.h,
"The regression (KernelSHAP) estimator", has the formulas; DESIGN.md 5f the reasoning):

* sizes: p(s) ~ 1 / (s (n - s)), s = 1 .. n-1, drawn by inverse CDF from ONE ``np.random.random_sample(S)`` on NumPy's global
  legacy generator; members: the first s_m entries of permutation m, the S permutations drawn after the sizes on the device from
  the same stream exactly as stage 1 draws its own (``hip_ops.sample_permutations``), the state handed back to the host;
* pairing (default): row 2m is S_m, row 2m+1 its complement, M = 2S rows;
* ``gram="sampled"``: A from the rows (the original KernelSHAP); ``gram="analytic"``: A is its expectation under the size law,
  only b comes from the rows (the unbiased variant of Covert & Lee);
* all 2^n - 2 proper coalitions with the weights of ``enumerated`` give the exact Shapley vector.

The moments and the solve run in libiq_hip.so (csrc/iq_kshap.hip): float64, fixed order, bitwise repeatable.
Games of 65 .. 1024 regions: wide_kernelshap.py (the analytic variant in closed form, on wide keep rows).
"""
import math
import sys

import numpy as np
import torch

from . import final_common, hip_ops, sparse_ops, work
from ._lib import IqError

MAX_REGIONS = hip_ops.MAX_KSHAP_REGIONS
GRAMS = ("sampled", "analytic")


regions = hip_ops.kshap_regions
_NARROW = sys.modules[__name__]      # what ``ks`` means in ``running_estimates`` and ``play`` unless wide_kernelshap.py is named


def check_gram(gram):
    if gram not in GRAMS:
        raise IqError("gram must be one of %s, got %r" % (GRAMS, gram))


def draws(samples, paired=True):
    """The coalitions to draw for ``samples`` rows: half of them, rounded down, when every one is followed by its complement."""
    s = int(samples) // 2 if paired else int(samples)
    if s < 1:
        raise IqError("samples=%d leaves no coalition to draw" % int(samples))
    return s


def end_rows(n, device):
    """The full and the empty coalition of n regions: the two rows ``rewards`` appends -> (2,) int64-typed."""
    return hip_ops.masks_to_tensor([(1 << n) - 1, 0], device)


def _size_cdf(n):
    """``size_cdf`` of any n >= 2, unchecked: shared with wide_kernelshap.py, whose range is another."""
    s = np.arange(1, n, dtype=np.float64)
    p = 1.0 / (s * (n - s))
    cdf = np.cumsum(p / p.sum())
    cdf[-1] = 1.0
    return cdf


def _draw_sizes(n, count):
    """``draw_sizes`` of any n >= 2, unchecked (wide_kernelshap.py)."""
    u = np.random.random_sample(int(count))
    return np.minimum(n - 1, 1 + np.searchsorted(_size_cdf(n), u, side="right")).astype(np.int32)


def size_cdf(n):
    """(n-1,) float64: entry s-1 = P(size <= s) under p(s) = (1 / (s (n - s))) / Z; the last entry is exactly 1.0."""
    return _size_cdf(regions(n))


def analytic_gram(n):
    """(n,n) float64: E[z z^T] under the size law - 1/2 on the diagonal, 1/2 - 1 / (2 H_{n-1}) off it."""
    n = regions(n)
    h = math.fsum(1.0 / k for k in range(1, n))
    a = np.full((n, n), 0.5 - 1.0 / (2.0 * h))
    np.fill_diagonal(a, 0.5)
    return a


def draw_sizes(n, count):
    """``count`` coalition sizes by the contract: one random_sample call on NumPy's global generator -> (count,) int32."""
    return _draw_sizes(regions(n), count)


def draw(n, samples, paired=True, device="cuda"):
    """One cloud's draw of ``samples`` rows (paired: rounded down to even, half of them drawn) -> (keep (M,) int64-typed device
    tensor, sizes (S,) int32 ndarray).  S doubles on the host, then S permutations on the device; NumPy's global generator is
    left where the reference's stream stands after both."""
    n = regions(n)
    s = draws(samples, paired)
    sizes = draw_sizes(n, s)
    state = hip_ops.mt_state_to_device(device)
    orders = hip_ops.sample_permutations(state, s, n)
    hip_ops.mt_state_to_host(state, set_global=True)
    return hip_ops.kshap_keep_masks(orders, torch.from_numpy(sizes).to(orders.device), paired), sizes


def enumeration_weights(n):
    """(n+1,) float64: entry s = w(S) of a coalition of s regions, (n-1) / (C(n,s) s (n-s)); 0 for the empty and the full set."""
    w = np.zeros(n + 1)
    for s in range(1, n):
        w[s] = (n - 1) / (math.comb(n, s) * s * (n - s))
    return w


def enumerated(n, device):
    """-> (keep (2^n - 2,) int64-typed, weights (2^n - 2,) float64), both on the device: every proper coalition of regions 0 .. n-1
    with the weight under which the regression returns the exact Shapley vector."""
    n = regions(n)
    if n > hip_ops.MAX_EXACT_PLAYERS:
        raise IqError("an enumerated game has 2^n rows: n=%d is above the limit of %d" % (n, hip_ops.MAX_EXACT_PLAYERS))
    count = (1 << n) - 2
    keep = hip_ops.enum_keep_masks(1, count, n, device)
    c = np.arange(1, count + 1, dtype=np.int64)
    size = np.zeros(count, dtype=np.int64)
    for k in range(n):
        size += (c >> k) & 1
    return keep, torch.from_numpy(enumeration_weights(n)[size]).to(keep.device)


def games(keep, v, v_empty, v_full):
    """What both ``estimate``s make of their rewards -> (v as a contiguous (G,M) tensor, v_empty (G,), v_full (G,) float64 on the
    device of ``keep``)."""
    if not isinstance(v, torch.Tensor) or v.dim() not in (1, 2):
        raise IqError("v must be a (M,) or (G,M) tensor")
    v2 = v.reshape(1, -1) if v.dim() == 1 else v
    ends = []
    for x, what in ((v_empty, "v_empty"), (v_full, "v_full")):
        t = torch.as_tensor(np.asarray(x.cpu() if isinstance(x, torch.Tensor) else x, dtype=np.float64).reshape(-1))
        if t.numel() != v2.shape[0]:
            raise IqError("%s holds %d values for %d games" % (what, t.numel(), v2.shape[0]))
        ends.append(t.to(keep.device))
    return v2.contiguous(), ends[0], ends[1]


def estimate(keep, v, v_empty, v_full, n, weights=None, gram="sampled"):
    """phi of the rows ``keep`` (M,) with rewards ``v`` ((M,) float32 device tensor, or (G,M) for G games on the same rows;
    v_empty, v_full: scalars or (G,)) -> float64 ndarray (n,) or (G,n).  IqError (hip_ops.KshapSingular) if the rows leave the
    sampled A singular."""
    n = regions(n)
    check_gram(gram)
    v2, v0, v1 = games(keep, v, v_empty, v_full)
    a, b, wsum = hip_ops.kshap_accum(keep, v2, v0, n, weights)
    a = a / wsum if gram == "sampled" else torch.from_numpy(analytic_gram(n)).to(keep.device)
    phi = hip_ops.kshap_solve(a.contiguous(), (b / wsum).contiguous(), v1 - v0).cpu().numpy()
    return phi[0] if v.dim() == 1 else phi


def pair_coefficients(n):
    """(n+1, 3) float64: row s = (alpha_s, beta_s, gamma_s) with mu(s, k) = alpha_s + beta_s k + gamma_s [k = 2] the SHAP-IQ
    weight of a row of s regions that holds k of a pair's two (include/iq.h, "All-pairs interactions from the regression rows"):
    alpha_s = 2 H s / (n - s - 1) (0 at s = n-1), beta_s = -2 H - alpha_s, gamma_s = 2 H (n - s) / (s - 1) + 4 H + alpha_s (0 at
    s = 1), rows 0 and n zero.  H = H_{n-1} is the float64 sum in ascending k of the contract; from it every entry is formed in
    rationals and rounded once.  Any n >= 2 (``hip_ops.kshap_pairs`` checks the range of a game)."""
    from fractions import Fraction
    n = int(n)
    if n < 2:
        raise IqError("a pair needs at least 2 regions, got %d" % n)
    h = 0.0
    for k in range(1, n):
        h += 1.0 / k
    two_h = 2 * Fraction(h)
    out = np.zeros((n + 1, 3))
    for s in range(1, n):
        alpha = two_h * s / (n - s - 1) if s <= n - 2 else Fraction(0)
        gamma = two_h * (n - s) / (s - 1) + 2 * two_h + alpha if s >= 2 else Fraction(0)
        out[s] = float(alpha), float(-two_h - alpha), float(gamma)
    return out


PAIR_PARTIAL_BYTES = 64 << 20     # kPairPartialBytes of csrc/iq_kshap_order.h


def chunks(m):
    """(count, tiles_per): the cut of m rows into chunks of whole 256-row tiles, at most 256 chunks - chunks_of of
    csrc/iq_kshap_order.h restated (the order of every moment; tests hold the two together through the scratch sizes)."""
    tiles = (int(m) + 255) // 256
    per = (tiles + 255) // 256
    return (tiles + per - 1) // per, per


def pair_chunks(m, n):
    """(count, tiles_per): the cut of the pairwise product's rows, ``chunks(m)`` with the count capped so that count * n * n
    float64 partials stay within PAIR_PARTIAL_BYTES (8 chunks at n = 1024) - pair_chunks_of of csrc/iq_kshap_order.h restated: a
    function of (m, n) alone."""
    count, per = chunks(m)
    cap = PAIR_PARTIAL_BYTES // (8 * int(n) * int(n))
    if count <= cap:
        return count, per
    tiles = (int(m) + 255) // 256
    per = (tiles + cap - 1) // cap
    return (tiles + per - 1) // per, per


def pairs(keep, v, v_empty, v_full, n, weights=None):
    """The SHAP-IQ estimate of the pairwise Shapley interaction index of ALL pairs of regions from the rows ``keep`` ((M,) narrow or
    (M,W) wide) with rewards ``v`` ((M,) float32 device tensor, or (G,M) for G games on the same rows; v_empty, v_full: scalars or
    (G,)) -> float64 ndarray (n,n) or (G,n,n), symmetric with a zero diagonal.  No further model evaluation: the rows are those
    ``estimate`` takes; with the enumerated rows and weights the result is the exact index."""
    v2, v0, v1 = games(keep, v, v_empty, v_full)
    out = hip_ops.kshap_pairs(keep, v2, v0, v1 - v0, n, weights).cpu().numpy()
    return out[0] if v.dim() == 1 else out


SE_NEEDS_SAMPLES = hip_ops.SE_NEEDS_SAMPLES
SE_NEEDS_ANALYTIC = ("the standard error of phi exists for gram='analytic' only: under the sampled Gram matrix phi is no mean of "
                     "independent units")


def pairs_se(keep, v, v_empty, v_full, n, paired=True, weights=None):
    """``pairs`` of SAMPLED rows with its standard error -> (interaction, se), float64 ndarrays (n,n) or (G,n,n): interaction the
    bits of ``pairs``, se symmetric with a zero diagonal.  An unbiased variance estimate from the second moment of the same rows
    over the iid units - a row, or ``paired`` a row and its complement - with no further model evaluation (include/iq.h,
    "Standard errors").  At least 2 units."""
    v2, v0, v1 = games(keep, v, v_empty, v_full)
    out, se = hip_ops.kshap_pairs_se(keep, v2, v0, v1 - v0, n, paired, weights)
    out, se = out.cpu().numpy(), se.cpu().numpy()
    return (out[0], se[0]) if v.dim() == 1 else (out, se)


CONTROLS = ("none", "shift", "regression")
LIST_CONTROLS = ("sparse",)     # the controls that take a pair list: offered beside CONTROLS at every region count
MAX_SPARSE_FEATURES = sparse_ops.MAX_FEATURES
CONTROL_NEEDS_PAIRS = "a control variate belongs to the all-pairs map: control=%r needs pairs=True"
RIDGE_SHARE = 64     # the default ridge of a fold's fit: its rows / 64 (a near-zero ridge is worse than no control)


def check_control(control):
    if control not in CONTROLS + LIST_CONTROLS:
        raise IqError("control must be one of %s, got %r" % (CONTROLS + LIST_CONTROLS, control))


def default_control_pairs(n):
    """The listed pairs of control="sparse" where the caller names none: min(3 n, 2080 - n) - the cells of a surface have about six
    neighbours, so 3 n pairs are about the adjacent ones; at 1024 regions the cap leaves 1056 - and never more than the
    n (n-1) / 2 pairs there are (below 7 regions)."""
    n = int(n)
    return min(3 * n, MAX_SPARSE_FEATURES - n, n * (n - 1) // 2)


def neighbour_pairs(centres, k):
    """The ``k`` pairs of regions (i < j) with the smallest squared distance between their centres ((R,3)) -> (k,2) int32, sorted
    row-major: a pair list of control="sparse".  The distance is float64 on the host, ties go to the lexicographically smaller
    (i, j).  It depends on the geometry only, never on a reward: the condition under which the sparse control is unbiased."""
    c = centres.detach().cpu().numpy() if isinstance(centres, torch.Tensor) else np.asarray(centres)
    c = np.asarray(c, dtype=np.float64)
    if c.ndim != 2 or c.shape[0] < 2:
        raise IqError("neighbour_pairs: centres must be (R,3) with R >= 2, got %s" % (tuple(c.shape),))
    r, k = c.shape[0], int(k)
    i, j = np.triu_indices(r, 1)                 # row-major over i < j: a stable sort keeps that order among ties
    if not 0 <= k <= len(i):
        raise IqError("neighbour_pairs: %d regions have %d pairs, k=%d" % (r, len(i), k))
    diff = c[i] - c[j]
    d2 = (diff * diff).sum(axis=1)
    pick = np.sort(np.argsort(d2, kind="stable")[:k])
    return np.stack([i[pick], j[pick]], axis=1).astype(np.int32).reshape(k, 2)


def fold_units(rows, paired=True):
    """(U_0, U_1): the units of the two contiguous folds of ``rows`` sampled rows, units [0, U/2) and [U/2, U) - a unit a row, or
    ``paired`` a row and its complement.  IqError unless both folds hold at least 2 whole units."""
    rows = int(rows)
    if paired and rows % 2:
        raise IqError("pairs_cv: %d paired rows are not whole pairs" % rows)
    u = rows // 2 if paired else rows
    if u < 4:
        raise IqError("pairs_cv: two folds of at least 2 units need 4 units, %d rows %s give %d" % (rows, "paired" if paired else "unpaired", u))
    return u // 2, u - u // 2


def pair_features(n):
    """d = n + n (n-1) / 2: the unknowns of the 2-additive surrogate (singles, then the pairs (i < j) row-major)."""
    return hip_ops.kshap_pair_features(n)


def fit_scratch_bytes(m, n, games):
    """The scratch of iq_kshap_pair_fit restated: A (d,d), the partials (G, chunks(m), d), the right-hand sides (G+1, d) and one
    float64, each rounded up to 256 bytes (tests hold it against the library's)."""
    d = int(n) + int(n) * (int(n) - 1) // 2
    up = lambda count: (8 * count + 255) // 256 * 256
    return up(d * d) + up(int(games) * chunks(m)[0] * d) + up((int(games) + 1) * d) + up(1)


def pair_coefficient_map(beta, n):
    """C(beta): (..., d) coefficients -> (..., n, n) float64, the pair coefficients mirrored, zero on the diagonal - the pair
    interactions of the 2-additive game the coefficients describe."""
    beta = np.asarray(beta, dtype=np.float64)
    out = np.zeros(beta.shape[:-1] + (n, n))
    i, j = np.triu_indices(n, 1)          # row-major over i < j: the order of the pair features
    out[..., i, j] = beta[..., n:]
    out[..., j, i] = beta[..., n:]
    return out


def sparse_coefficient_map(beta, n, pair_list):
    """C(beta) of a sparse surrogate: (..., n + K) coefficients -> (..., n, n) float64, beta_{n+k} at (i_k, j_k) and (j_k, i_k), 0
    elsewhere."""
    beta = np.asarray(beta, dtype=np.float64)
    out = np.zeros(beta.shape[:-1] + (n, n))
    i, j = pair_list[:, 0].astype(np.int64), pair_list[:, 1].astype(np.int64)
    out[..., i, j] = beta[..., n:]
    out[..., j, i] = beta[..., n:]
    return out


def pairs_cv(keep, v, v_empty, v_full, n, paired=True, control="regression", ridge=None, weights=None, pair_list=None):
    """The control-variate estimate of the all-pairs Shapley interaction index from SAMPLED rows, with its standard error, on the
    rows and rewards ``pairs_se`` takes and with no further model evaluation -> (interaction, se, info): float64 ndarrays (n,n)
    or (G,n,n), symmetric bit for bit with a zero diagonal, and a dict (include/iq.h, "Control variates for the all-pairs map";
    DESIGN.md 5j).

    ``control="shift"`` (2 .. 1024 regions, narrow or wide rows): SHAP-IQ on the rewards less the additive game delta s / n.
    ``control="regression"`` (2 .. 64 regions, narrow rows): two contiguous folds of units; a 2-additive surrogate is fitted to
    each fold (ridge ``ridge``, default a fold's rows / 64, under sum(beta) = delta), its pair coefficients are read off and SHAP-IQ
    runs on the OTHER fold's residuals; the two estimates are averaged by rows.  Unbiased whatever the fit; the standard error
    neglects the covariance between the folds.  info: control, paired, fold_rows, ridge (per fold), status, beta ((2,G,d) or
    (2,d)) - for the shift fold_rows is the one range of rows and ridge, beta are None.

    ``control="sparse"`` (2 .. 1024 regions, narrow or wide rows): the regression control with a surrogate of all n
    singles and the K pairs of ``pair_list`` ((K,2), 0 <= i < j < n, strictly increasing row-major, n + K <= 2080; K = 0: a
    fitted additive control; the complete list at n <= 64: ``regression`` bit for bit).  Unbiased whatever the list, PROVIDED
    the list does not depend on the rewards of these rows (``neighbour_pairs`` depends on geometry only).  info gains "pairs",
    the (K,2) int32 list, and "features", d = n + K."""
    check_control(control)
    if (pair_list is not None) != (control in LIST_CONTROLS):
        raise IqError("pairs_cv: pair_list belongs to control='sparse' and control='sparse' needs one, got control=%r with%s a list"
                      % (control, "out" if pair_list is None else ""))
    if control == "none":
        raise IqError("pairs_cv: control='none' is pairs_se")
    if weights is not None:
        raise IqError("pairs_cv: " + hip_ops.SE_NEEDS_SAMPLES)
    v2, v0, v1 = games(keep, v, v_empty, v_full)
    delta = v1 - v0
    single = v.dim() == 1
    m = keep.shape[0]
    if control == "shift":
        t = hip_ops.kshap_pair_shift_terms(keep, v2, v0, delta, n)
        out, se = hip_ops.kshap_pairs_terms_se(keep, t, n, paired)
        out, se = out.cpu().numpy(), se.cpu().numpy()
        info = {"control": control, "paired": bool(paired), "fold_rows": [m], "ridge": None, "status": 0, "beta": None}
        return (out[0], se[0], info) if single else (out, se, info)
    sparse = control in LIST_CONTROLS
    if sparse:
        pair_list = sparse_ops.check_pair_list(pair_list, n)
        d = int(n) + len(pair_list)
    else:
        d = pair_features(n)                  # refuses more than 64 regions, naming the shift and the sparse control
    n = int(n)
    if ridge is not None and not float(ridge) >= 0.0:
        raise IqError("pairs_cv: ridge must be a number >= 0, got %r" % (ridge,))
    u0, u1 = fold_units(m, paired)
    c = 2 if paired else 1
    cuts = ((0, c * u0), (c * u0, c * (u0 + u1)))
    rows = [hi - lo for lo, hi in cuts]
    kf = [keep[lo:hi].contiguous() for lo, hi in cuts]
    vf = [v2[:, lo:hi].contiguous() for lo, hi in cuts]
    ridges = [rows[f] / float(RIDGE_SHARE) if ridge is None else float(ridge) for f in range(2)]
    if sparse:
        ff = [sparse_ops.kshap_sparse_expand(kf[f], pair_list, n) for f in range(2)]
        beta = [sparse_ops.kshap_feat_fit(sparse_ops.kshap_feat_gram(ff[f], d), ff[f], vf[f], v0, delta, d, ridges[f]) for f in range(2)]
    else:
        beta = [hip_ops.kshap_pair_fit(hip_ops.kshap_pair_gram(kf[f], n), kf[f], vf[f], v0, delta, n, ridges[f]) for f in range(2)]
    est, var = [], []
    for f in range(2):
        other = beta[1 - f]
        if sparse:
            _, t = sparse_ops.kshap_feat_surrogate(ff[f], other, d, vf[f], v0)
        else:
            _, t = hip_ops.kshap_pair_surrogate(kf[f], other, n, vf[f], v0)
        res, se_f = hip_ops.kshap_pairs_terms_se(kf[f], t, n, paired)
        b = other.cpu().numpy()
        slack = (delta.cpu().numpy() - b.sum(axis=1)) / (n - 1)          # the rounding of the efficiency constraint
        i_f = (sparse_coefficient_map(b, n, pair_list) if sparse else pair_coefficient_map(b, n)) + res.cpu().numpy()
        i_f[:, ~np.eye(n, dtype=bool)] += slack[:, None]
        est.append(i_f)
        var.append(se_f.cpu().numpy() ** 2)
    total = float(rows[0] + rows[1])
    out = (rows[0] * est[0] + rows[1] * est[1]) / total
    se = np.sqrt(rows[0] ** 2 * var[0] + rows[1] ** 2 * var[1]) / total
    betas = np.stack([b.cpu().numpy() for b in beta])
    info = {"control": control, "paired": bool(paired), "fold_rows": rows, "ridge": ridges, "status": 0,
            "beta": betas[:, 0] if single else betas}
    if sparse:
        info.update(pairs=pair_list, features=d)
    return (out[0], se[0], info) if single else (out, se, info)


def phi_se(keep, v, v_empty, v_full, n, paired=True, gram="analytic", ks=_NARROW, weights=None):
    """``ks.estimate`` of SAMPLED rows under the analytic Gram matrix with its standard error -> (phi, se), float64 ndarrays (n,)
    or (G,n): phi the bits of ``estimate``, se = sqrt(max(var, 0)) of ``hip_ops.kshap_moment_se``.  ``gram="sampled"`` is refused."""
    n = ks.regions(n)
    ks.check_gram(gram)
    if gram != "analytic":
        raise IqError(SE_NEEDS_ANALYTIC)
    if weights is not None:
        raise IqError(SE_NEEDS_SAMPLES)
    phi = ks.estimate(keep, v, v_empty, v_full, n, None, gram)
    v2, v0, _ = games(keep, v, v_empty, v_full)
    var = hip_ops.kshap_moment_se(keep, v2, v0, n, paired)[1].cpu().numpy()
    se = np.sqrt(np.maximum(var, 0.0))
    return phi, (se[0] if v.dim() == 1 else se)


def default_samples(n):
    """Stage 1's budget of model evaluations: 1000 permutations of n + 1 prefix coalitions, rounded down to even."""
    return 1000 * (n + 1) // 2 * 2


def running_counts(n, rows, paired=True, counts=None):
    """The row counts at which ``shapley`` reports a running estimate: c (n + 1) for c in shapley_stage.SAMPLE_NUMS (the model
    evaluations of c permutations), rounded down to even when paired, that do not exceed ``rows``."""
    if counts is None:
        from .shapley_stage import SAMPLE_NUMS
        counts = [c * (n + 1) for c in SAMPLE_NUMS]
    counts = [int(c) // 2 * 2 if paired else int(c) for c in counts]
    return [c for c in counts if 1 <= c <= rows]


def rewards(model, data, lbl, region_id, args, keep, chunk=1 << 16, classes=None):
    """Rewards of the coalitions ``keep`` of one cloud ``data`` (1,N,3), obtained as exact.value_table obtains them, with the
    full and the empty coalition as two extra rows of the same calls (final_common.rewards_with_ends) -> (v (M,) float32 device
    tensor, v_full, v_empty).  ``classes`` (a sequence of labels, or "all"; ``lbl`` is then not read): the rewards of every
    label from the same logits -> (v (G,M), v_full (G,), v_empty (G,)), row g the bits of the call with lbl = classes[g]."""
    if not hasattr(model, "coalition_logits"):
        raise IqError("%s has no coalition entry point" % type(model).__name__)
    r = regions(args.num_regions)
    rid = hip_ops.region_ids(region_id, data.device, r).reshape(1, -1)
    clouds = data.contiguous()
    centers = torch.mean(data, dim=1).reshape(1, 3).contiguous()

    def logits_of(part):
        work.add(part.numel())
        return model.coalition_logits(clouds, centers, rid, part, None, num_regions=r, validate=False)
    return final_common.rewards_with_ends(logits_of, keep, end_rows(r, data.device), lbl, classes, args, chunk)


def running_estimates(keep, v, v_empty, v_full, n, counts, gram="sampled", ks=_NARROW):
    """{count: ``ks.estimate`` of the first ``count`` rows}; a count whose rows leave the sampled A singular is left out (the
    wide estimator has no such case: every count is there)."""
    out = {}
    for c in counts:
        try:
            out[c] = ks.estimate(keep[:c].contiguous(), v[:c].contiguous(), v_empty, v_full, n, None, gram)
        except hip_ops.KshapSingular:
            pass
    return out


def play(ks, model, data, lbl, region_id, args, samples=None, paired=True, gram="sampled", counts=None, draw=None, classes=None,
         pairs=False, se=False, control="none", control_pairs=None, centres=None, **how):
    """The body of ``game``, wide_kernelshap.game and classwise.kernel_shapley, which check their own arguments first.  ``ks``:
    the estimator's module, this one or wide_kernelshap.  Refused before anything is drawn or run: the region count and
    ``gram``.  Then the rows - ``samples`` a count, None (``ks.default_samples``) or "all" (``ks.enumerated``); ``draw``:
    (n, samples, paired, device) -> (keep, sizes), default ``ks.draw`` - their rewards (``ks.rewards`` with ``classes`` and
    ``how``), ``ks.estimate`` and the running estimates at ``ks.running_counts`` (``counts=()``: none) -> the dict ``game``
    describes; ``pairs``: also "interaction", ``ks.pairs`` of the same rows and rewards ((n,n), or (G,n,n) with ``classes``; no
    running estimates of it).  ``se``: also the standard errors of the sampled estimates, "phi_se" under the analytic Gram matrix
    and "interaction_se" with ``pairs``; refused before anything is drawn with ``samples="all"`` and where neither exists (the
    sampled Gram matrix without ``pairs``).  ``control`` other than "none" (with ``pairs``, sampled rows): also
    "interaction_cv", "interaction_cv_se" and "control" (the info dict) of ``ks.pairs_cv`` on the same rows; everything else is
    what it is without it.  ``control="sparse"`` takes ``control_pairs``: a pair list, or a count k (None:
    ``default_control_pairs``) - then ``neighbour_pairs`` of ``centres`` (n,3), the FPS centres of the regions; the list is checked
    before anything is drawn."""
    n = ks.regions(args.num_regions)
    ks.check_gram(gram)
    check_control(control)
    if control != "none":
        if not pairs:
            raise IqError(CONTROL_NEEDS_PAIRS % control)
        if isinstance(samples, str):
            raise IqError(SE_NEEDS_SAMPLES)
        if control not in ks.CONTROLS + ks.LIST_CONTROLS:
            raise IqError("control=%r is not available for %d regions here: one of %s" % (control, n, ks.CONTROLS + ks.LIST_CONTROLS))
    if control_pairs is not None and control not in LIST_CONTROLS:
        raise IqError("control_pairs belongs to control='sparse', got control=%r" % (control,))
    pair_list = None
    if control in LIST_CONTROLS:
        if control_pairs is None or isinstance(control_pairs, (int, np.integer)):
            k = default_control_pairs(n) if control_pairs is None else int(control_pairs)
            if k < 0 or k > min(MAX_SPARSE_FEATURES - n, n * (n - 1) // 2):
                raise IqError("control_pairs=%d: 0 .. %d pairs beside %d regions" % (k, min(MAX_SPARSE_FEATURES - n, n * (n - 1) // 2), n))
            if centres is None or len(centres) != n:
                raise IqError("control='sparse' with a count of pairs needs centres (%d,3): the FPS centres of the regions" % n)
            control_pairs = neighbour_pairs(centres, k)
        pair_list = sparse_ops.check_pair_list(control_pairs, n)
    if se and isinstance(samples, str):
        raise IqError(SE_NEEDS_SAMPLES)
    if se and gram != "analytic" and not pairs:
        raise IqError(SE_NEEDS_ANALYTIC)
    weights = None
    if isinstance(samples, str):
        if samples != "all":
            raise IqError("samples must be a count, None or 'all', got %r" % (samples,))
        keep, weights = ks.enumerated(n, data.device)
    else:
        keep, _ = (draw or ks.draw)(n, ks.default_samples(n) if samples is None else samples, paired, data.device)
    v, v_full, v_empty = ks.rewards(model, data, lbl, region_id, args, keep, classes=classes, **how)
    phi = ks.estimate(keep, v, v_empty, v_full, n, weights, gram)
    running = {}
    if weights is None:
        running = running_estimates(keep, v, v_empty, v_full, n, ks.running_counts(n, keep.shape[0], paired, counts), gram, ks)
    out = {"keep": keep, "weights": weights, "v": v, "v_full": v_full, "v_empty": v_empty, "phi": phi, "running": running}
    if pairs and se:
        out["interaction"], out["interaction_se"] = ks.pairs_se(keep, v, v_empty, v_full, n, paired)
    elif pairs:
        out["interaction"] = ks.pairs(keep, v, v_empty, v_full, n, weights)
    if se and gram == "analytic":
        out["phi_se"] = ks.phi_se(keep, v, v_empty, v_full, n, paired, gram)[1]
    if control != "none":
        out["interaction_cv"], out["interaction_cv_se"], out["control"] = ks.pairs_cv(
            keep, v, v_empty, v_full, n, paired, control, **({"pair_list": pair_list} if pair_list is not None else {}))
    return out


def game(model, data, lbl, region_id, args, samples=None, paired=True, gram="sampled", counts=None, pairs=False, se=False,
         control="none", control_pairs=None, centres=None):
    """One cloud's sampled (or enumerated) game with everything the driver stores: dict of keep (M,), weights (None when
    sampled), v (M,) float32 rewards, v_full, v_empty, phi (n,) and running {count: phi of the first ``count`` rows};
    ``pairs``: also interaction (n,n), ``pairs`` of the same rows; ``se``: also phi_se (n,) under the analytic Gram matrix and,
    with ``pairs``, interaction_se (n,n); ``control``: also interaction_cv, interaction_cv_se (n,n) and control (``play``, which
    describes ``control_pairs`` and ``centres`` of control="sparse").  A
    ``gram`` outside GRAMS is refused before anything is drawn or run."""
    return play(_NARROW, model, data, lbl, region_id, args, samples, paired, gram, counts, pairs=pairs, se=se, control=control,
                control_pairs=control_pairs, centres=centres)


def shapley(model, data, lbl, region_id, args, samples=None, paired=True, gram="sampled", counts=None):
    """-> (phi (n,) float64 ndarray, v_full, v_empty, running {count: (n,) phi of the first ``count`` rows}) of one cloud.
    ``samples``: rows to draw (None: default_samples(n)), or "all": the enumerated game, exact up to rounding (no running
    estimates)."""
    g = game(model, data, lbl, region_id, args, samples, paired, gram, counts)
    return g["phi"], g["v_full"], g["v_empty"], g["running"]


def from_table(v_table, keep, weights=None, gram="sampled"):
    """The estimate of the rows ``keep`` with rewards read off an exact value table (exact.value_table; players are regions
    0 .. n-1, so a coalition's reward is v_table[keep]) - the counterpart of exact.sampled_from_table -> (n,) float64 ndarray."""
    n = int(v_table.numel()).bit_length() - 1
    if v_table.dim() != 1 or v_table.numel() != 1 << n:
        raise IqError("v_table must be a (2^n,) table, got shape %s" % (tuple(v_table.shape),))
    ends = v_table[[0, v_table.numel() - 1]].cpu().numpy()
    return estimate(keep, v_table.index_select(0, keep).contiguous(), float(ends[0]), float(ends[1]), n, weights, gram)


def pairs_from_table(v_table, keep, weights=None):
    """``pairs`` of the rows ``keep`` with rewards read off an exact value table, as ``from_table`` reads them -> (n,n) float64."""
    n = int(v_table.numel()).bit_length() - 1
    if v_table.dim() != 1 or v_table.numel() != 1 << n:
        raise IqError("v_table must be a (2^n,) table, got shape %s" % (tuple(v_table.shape),))
    ends = v_table[[0, v_table.numel() - 1]].cpu().numpy()
    return pairs(keep, v_table.index_select(0, keep).contiguous(), float(ends[0]), float(ends[1]), n, weights)
