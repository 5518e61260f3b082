"""NumPy restatement of the standard errors of the sampled estimates (include/iq.h, "Standard errors"), straight from
the DEFINING formulas: a unit u is the iid draw - a row, or (paired) a row and its complement - and for an estimate
est = const + (1/M) sum_u y_u

    var = (U / (U - 1)) (sum y_u^2 - (sum y_u)^2 / U) / M^2.

For a pair {i,j} y_u is the unit's SHAP-IQ term x_u(k), k the number of the pair's members in the unit's first row, with mu from
exact rationals (kshap_pairs_ref.mu) and the three cases k = 2, 1, 0 squared and summed on their own over z and 1 - z - not the
one-product form the library computes.  For phi under the analytic Gram matrix y_ui = 2 H D_u (z_ui - s_u / R), formed and squared
entry by entry.  Sums over the units: ``kshap_pairs_ref.pair_sums`` (exact to 2^-76 of the largest term) for the pairs, extended
precision for phi.  ``exact_moments`` enumerates the law of a unit in rationals: the mean and the variance every estimate is held
against.  It shares no code with interpret_quality_amd/kernelshap.py."""
from fractions import Fraction
from itertools import combinations
from math import comb

import numpy as np

import kshap_pairs_ref as pairs_ref

L = np.longdouble


def _long(x):
    return L(x.numerator) / L(x.denominator)


def first_rows(keep, r, paired):
    """keep (M,) or (M,W) -> (U,R) uint8: the first row of every unit."""
    z = pairs_ref.rows_of(keep, r)
    if paired and len(z) % 2:
        raise ValueError("paired rows come in twos")
    return z[::2] if paired else z


def unit_terms(keep, v, v0, r, paired):
    """-> (x (U,3) longdouble, z (U,R) uint8): x[u][k] = x_u(k), the unit's term for a pair with k members in its first row z[u]:
    d_u mu(s,k), or paired d_2u mu(s,k) + d_2u+1 mu(R-s, 2-k); 0 for a first row of size 0 or R (mu's rows 0 and R are 0)."""
    z = first_rows(keep, r, paired)
    _, d = pairs_ref.terms(v, v0, None, len(np.asarray(v).reshape(-1)))
    d = d.astype(L)
    mu = pairs_ref._as_long(pairs_ref.mu(r))
    s = z.sum(axis=1, dtype=np.int64)
    if not paired:
        return d[:, None] * mu[s], z
    x = d[0::2, None] * mu[s] + d[1::2, None] * mu[r - s][:, ::-1]
    x[(s == 0) | (s == r)] = 0
    return x, z


def _by_cases(z, y):
    """z (U,R) uint8, y (U,3) longdouble -> (R,R) longdouble: sum_u y[u][k_ij(u)], the three cases on their own."""
    zf = z.astype(np.float64)
    zc = 1.0 - zf
    one = pairs_ref.pair_sums(zf, zc, y[:, 1])
    return pairs_ref.pair_sums(zf, zf, y[:, 2]) + (one + one.T) + pairs_ref.pair_sums(zc, zc, y[:, 0])


def pairs_moments(keep, v, v0, r, paired):
    """-> (S1 (R,R), S2 (R,R)) longdouble: sum_u x_u(k_ij) and sum_u x_u(k_ij)^2; the diagonal is not an estimate."""
    x, z = unit_terms(keep, v, v0, r, paired)
    return _by_cases(z, x), _by_cases(z, x * x)


def variance(s1, s2, units, rows):
    """(U / (U - 1)) (S2 - S1^2 / U) / M^2 in extended precision."""
    u, m = L(units), L(rows)
    return (u / (u - 1)) * (s2 - s1 * s1 / u) / (m * m)


def pairs_var(keep, v, v0, r, paired):
    """(R,R) float64: the variance estimate of every I_ij of one game, zero diagonal."""
    s1, s2 = pairs_moments(keep, v, v0, r, paired)
    rows = len(np.asarray(v).reshape(-1))
    out = variance(s1, s2, rows // 2 if paired else rows, rows).astype(np.float64)
    np.fill_diagonal(out, 0.0)
    return out


def phi_units(keep, v, v0, r, paired):
    """(U,R) longdouble: y_ui = 2 H D_u (z_ui - s_u / R), D_u = d_u or d_2u - d_2u+1, H exact."""
    z = first_rows(keep, r, paired)
    _, d = pairs_ref.terms(v, v0, None, len(np.asarray(v).reshape(-1)))
    d = d.astype(L)
    big_d = d[0::2] - d[1::2] if paired else d
    s = z.sum(axis=1, dtype=np.int64).astype(L)
    return 2 * _long(pairs_ref.harmonic(r)) * big_d[:, None] * (z.astype(L) - (s / L(r))[:, None])


def phi_moments(keep, v, v0, r, paired):
    y = phi_units(keep, v, v0, r, paired)
    return y.sum(axis=0), (y * y).sum(axis=0)


def phi_var(keep, v, v0, r, paired):
    """(R,) float64: the variance estimate of phi_i = delta / R + (1/M) sum_u y_ui."""
    s1, s2 = phi_moments(keep, v, v0, r, paired)
    rows = len(np.asarray(v).reshape(-1))
    return variance(s1, s2, rows // 2 if paired else rows, rows).astype(np.float64)


def shapley_se(total, sq, n):
    """The permutation estimator: sqrt(max(sq - total^2 / n, 0) / (n (n - 1)))."""
    return np.sqrt(np.maximum(sq - total * total / n, 0.0) / (n * (n - 1)))


# ---- the law of a unit, enumerated in rationals (small R) -------------------------------------------------------------------------

def unit_law(r):
    """[(P(S), S as a bitmask)] over the proper coalitions: p(s) / C(R,s), p(s) = 1 / (s (R - s) Z), Z = 2 H / R."""
    z = 2 * pairs_ref.harmonic(r) / r
    out = []
    for s in range(1, r):
        p = 1 / (s * (r - s) * z) / comb(r, s)
        for members in combinations(range(r), s):
            out.append((p, sum(1 << i for i in members)))
    assert sum(p for p, _ in out) == 1
    return out


def pair_term(table, mask, i, j, r, paired, independent=False):
    """x_u of the pair {i,j} for the unit whose first row is ``mask``, in rationals; ``table``: the (2^R,) integer value table.
    ``independent``: the WRONG reading of a paired unit - its second row taken as a draw of its own - returns the two rows' terms
    apart, (first, second)."""
    mu = pairs_ref.mu(r)
    full = (1 << r) - 1
    v0 = int(table[0])

    def term(m):
        s, k = bin(m).count("1"), (m >> i & 1) + (m >> j & 1)
        return (int(table[m]) - v0) * mu[s, k]
    if not paired:
        return term(mask)
    return (term(mask), term(full & ~mask)) if independent else term(mask) + term(full & ~mask)


def phi_term(table, mask, i, r, paired):
    """y_ui for the unit whose first row is ``mask``, in rationals."""
    full = (1 << r) - 1
    v0 = int(table[0])
    d = int(table[mask]) - v0 - ((int(table[full & ~mask]) - v0) if paired else 0)
    return 2 * pairs_ref.harmonic(r) * d * ((mask >> i & 1) - Fraction(bin(mask).count("1"), r))
