"""NumPy restatement of the control-variate estimators of the all-pairs map (include/iq.h, "Control variates for the all-pairs
map"), straight from the DEFINING formulas: the features as subset tests on Python integers, the Gram matrix as
integer counts, the surrogate as a longdouble product, and SHAP-IQ on per-row terms through tests/kshap_pairs_ref.py and
tests/kshap_se_ref.py by import - a term t_m is handed to them as the float64 reward of a game with v0 = 0 and delta = 0, which
makes d_m = t_m exactly and the delta term 0.  The fit is NumPy's float64 solve of the bordered (KKT) system, not a Cholesky
factor and not the two-solve form the library computes.  It shares no code with interpret_quality_amd/kernelshap.py."""
import numpy as np

import kshap_pairs_ref as pairs_ref
import kshap_se_ref as se_ref

L = np.longdouble
U = 2.0 ** -53


def feature_count(r):
    return r + r * (r - 1) // 2


def feature_masks(r):
    """[fm_a]: the singles, then the pairs (i < j) in row-major order, as Python integers."""
    return [1 << i for i in range(r)] + [(1 << i) | (1 << j) for i in range(r) for j in range(i + 1, r)]


def features_by_masks(keep, r):
    """keep (M,) uint64 narrow rows -> (M,d) uint8: f_a(S_m) = [fm_a subset of S_m], the definition on Python integers; bits at or
    above r play no part."""
    rows = [int(k) & ((1 << r) - 1) for k in np.asarray(keep).reshape(-1)]
    return np.array([[1 if k & fm == fm else 0 for fm in feature_masks(r)] for k in rows], dtype=np.uint8).reshape(len(rows), feature_count(r))


def features(keep, r):
    """The same (M,d) uint8 matrix from the rows' bits: the singles are the bits, a pair's feature the product of its two
    (tests/test_kshap_paircv_cpu.py holds it against ``features_by_masks``)."""
    z = pairs_ref.rows_of(np.asarray(keep).reshape(-1, 1), r)
    i, j = np.triu_indices(r, 1)                      # row-major over i < j
    return np.concatenate([z, z[:, i] & z[:, j]], axis=1)


def gram(keep, r):
    """(d,d) int64: the number of rows that hold feature a and feature b (a float64 product of 0/1 matrices: every partial sum an
    integer below 2^53, exact in any order)."""
    f = features(keep, r).astype(np.float64)
    out = f.T @ f
    assert out.max(initial=0.0) < 2.0 ** 53
    return out.astype(np.int64)


def rhs(keep, v, v0, r):
    """(d,) longdouble: sum_m f_a(S_m) ((double)v_m - v0) of one game."""
    d = np.asarray(v).astype(np.float64) - float(v0)
    return features(keep, r).astype(L).T @ d.astype(L)


def fit(keep, v, v0, delta, r, ridge):
    """beta (d,) float64 of one game: min |F beta - d|^2 + ridge |beta|^2 subject to sum(beta) = delta, from the bordered system
    [[A, 1], [1^T, 0]] [beta; lambda] = [c; delta]."""
    d = feature_count(r)
    k = np.zeros((d + 1, d + 1))
    k[:d, :d] = gram(keep, r).astype(np.float64) + float(ridge) * np.eye(d)
    k[:d, d] = k[d, :d] = 1.0
    return np.linalg.solve(k, np.concatenate([rhs(keep, v, v0, r).astype(np.float64), [float(delta)]]))[:d]


def surrogate(keep, beta, r):
    """(M,) longdouble: g_beta(S_m)."""
    return features(keep, r).astype(L) @ np.asarray(beta, dtype=np.float64).astype(L)


def pair_map(beta, r):
    """C(beta) (r,r): the pair coefficients mirrored, zero diagonal."""
    out = np.zeros((r, r))
    a = r
    for i in range(r):
        for j in range(i + 1, r):
            out[i, j] = out[j, i] = beta[a]
            a += 1
    return out


def sizes(keep, r):
    return pairs_ref.rows_of(keep, r).sum(axis=1, dtype=np.int64)


def shift_terms(keep, v, v0, delta, r):
    """(M,) float64: ((double)v - v0) - (delta s) / r, every operation rounded on its own."""
    return (np.asarray(v).astype(np.float64) - float(v0)) - (float(delta) * sizes(keep, r).astype(np.float64)) / float(r)


def residual_terms(keep, v, v0, beta, r):
    """(M,) float64: ((double)v - v0) - g_beta(S_m), the surrogate in extended precision, rounded once."""
    return ((np.asarray(v).astype(np.float64) - float(v0)).astype(L) - surrogate(keep, beta, r)).astype(np.float64)


def shapiq(keep, t, r, weights=None):
    """(r,r) float64: SHAP-IQ on the terms t, with no delta term (kshap_pairs_ref.pairs of the game v = t, v0 = 0, delta = 0)."""
    return pairs_ref.pairs(keep, np.asarray(t, dtype=np.float64), 0.0, 0.0, r, weights)


def shapiq_var(keep, t, r, paired):
    """(r,r) float64: the variance estimate of ``shapiq`` over the units (kshap_se_ref.pairs_var on the same game)."""
    return se_ref.pairs_var(keep, np.asarray(t, dtype=np.float64), 0.0, r, paired)


def bound(keep, t, r, weights=None):
    """kshap_pairs_ref.bound computed on the terms."""
    return pairs_ref.bound(keep, np.asarray(t, dtype=np.float64), 0.0, r, weights)


def with_surrogate(keep, v, v0, delta, beta, r, weights=None):
    """C(beta) + (delta - sum(beta)) / (r-1) + SHAPIQ(v - v0 - g_beta): the estimate of the index given ANY beta (the middle term
    is the share of the full set, which the residual game of a beta that does not sum to delta still has) -> ((r,r), terms)."""
    t = residual_terms(keep, v, v0, beta, r)
    out = pair_map(beta, r) + shapiq(keep, t, r, weights)
    slack = float((L(float(delta)) - np.asarray(beta, dtype=np.float64).astype(L).sum()) / L(r - 1))
    out[~np.eye(r, dtype=bool)] += slack
    return out, t


def fold_rows(rows, paired):
    """((lo, hi), (lo, hi)): the rows of the two contiguous folds, units [0, U/2) and [U/2, U)."""
    c = 2 if paired else 1
    units = rows // c
    return (0, c * (units // 2)), (c * (units // 2), c * units)


def pairs_cv(keep, v, v0, delta, r, paired=True, control="regression", ridge=None):
    """-> (I (r,r), se (r,r)) float64 of one game by the contract."""
    keep = np.asarray(keep).reshape(len(keep), -1)
    v = np.asarray(v)
    if control == "shift":
        t = shift_terms(keep, v, v0, delta, r)
        return shapiq(keep, t, r), np.sqrt(np.maximum(shapiq_var(keep, t, r, paired), 0.0))
    cuts = fold_rows(len(keep), paired)
    beta = [fit(keep[lo:hi, 0], v[lo:hi], v0, delta, r, (hi - lo) / 64.0 if ridge is None else ridge) for lo, hi in cuts]
    est, var, rows = [], [], []
    for f, (lo, hi) in enumerate(cuts):
        i_f, t = with_surrogate(keep[lo:hi], v[lo:hi], v0, delta, beta[1 - f], r)
        est.append(i_f)
        var.append(shapiq_var(keep[lo:hi], t, r, paired))
        rows.append(hi - lo)
    m = float(rows[0] + rows[1])
    out = (rows[0] * est[0] + rows[1] * est[1]) / m
    return out, np.sqrt(np.maximum(rows[0] ** 2 * var[0] + rows[1] ** 2 * var[1], 0.0)) / m
