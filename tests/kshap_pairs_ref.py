"""NumPy restatement of the all-pairs interaction estimator's contract (include/iq.h, "All-pairs interactions from the regression
rows"), straight from the DEFINING formula

    I_ij = delta / (R - 1) + (1 / W_sum) sum_m d_m mu(s_m, z_mi + z_mj),      d_m = w_m ((double)v_m - v0),

with mu from exact rationals (exact H_{R-1} too) and the three cases k = 2, 1, 0 summed on their own over z and 1 - z - not the
alpha/beta/gamma form the library computes.  Every sum over the rows is exact to 2^-76 of its largest term (``pair_sums``: the
limb construction of wide_kernelshap_ref.exact_sums, against which tests/test_kshap_pairs_cpu.py holds it), so the restatement
carries no summation order and no cancellation of its own.  It shares no code with interpret_quality_amd/kernelshap.py."""
from fractions import Fraction

import numpy as np

import wide_kernelshap_ref as wide

U = 2.0 ** -53
L = np.longdouble


def harmonic(r):
    """H_{R-1}, exact."""
    return sum(Fraction(1, k) for k in range(1, r))


def mu(r):
    """(R+1, 3) Fractions: entry [s][k] = mu(s, k) = gamma(s,k) C(R,s) / p(s) in closed form; 0 where no pair can meet it (k = 2 at
    s < 2, k = 0 at s > R - 2) and in rows 0 and R, which contribute nothing."""
    h2 = 2 * harmonic(r)
    out = np.full((r + 1, 3), Fraction(0), dtype=object)
    for s in range(1, r):
        if s <= r - 2:
            out[s, 0] = h2 * s / (r - s - 1)
        out[s, 1] = -h2
        if s >= 2:
            out[s, 2] = h2 * (r - s) / (s - 1)
    return out


def mu_from_gamma(r):
    """The same table from the definition, gamma(s,k) C(R,s) / p(s) with factorials - the check of the closed form (small R)."""
    from math import comb, factorial
    z = 2 * harmonic(r) / r
    out = np.full((r + 1, 3), Fraction(0), dtype=object)
    for s in range(1, r):
        p = 1 / (s * (r - s) * z)
        for k in range(3):
            if s - k >= 0 and r - s - 2 + k >= 0:
                out[s, k] = Fraction((-1) ** k * factorial(s - k) * factorial(r - s - 2 + k), factorial(r - 1)) * comb(r, s) / p
    return out


def coefficients(r):
    """(R+1, 3) Fractions (alpha_s, beta_s, gamma_s) with mu(s,k) = alpha + beta k + gamma [k = 2], by the contract's choices:
    alpha_{R-1} = 0, gamma_1 = 0, rows 0 and R zero."""
    m = mu(r)
    out = np.full((r + 1, 3), Fraction(0), dtype=object)
    for s in range(1, r):
        a = m[s, 0]
        out[s] = a, m[s, 1] - a, (m[s, 2] - 2 * m[s, 1] + a) if s >= 2 else Fraction(0)
    return out


def _as_float(table):
    return np.array([[float(x) for x in row] for row in table], dtype=np.float64)


def _as_long(table):
    return np.array([[L(x.numerator) / L(x.denominator) for x in row] for row in table], dtype=L)


def rows_of(keep, r):
    """keep (M,) narrow or (M,W) wide -> (M,R) uint8 rows z."""
    return wide.bits(np.asarray(keep).reshape(len(keep), -1), r)


def terms(v, v0, weights, m):
    """-> (w (M,), d (M,)) of ONE game: the float64 terms the contract names (wide_kernelshap_ref._terms)."""
    w, d = wide._terms(np.asarray(v).reshape(-1), [float(v0)], weights, m)
    return w, d[:, 0]


BITS = 76      # of every term below the largest term's leading bit that the sums keep: what is cut off is below 2^-76 of it


def pair_sums(za, zb, x):
    """za, zb (M,R) 0/1 float64, x (M,) longdouble -> (R,R) longdouble sum_m x_m za[m,i] zb[m,j], exact but for 2^-BITS max|x| per
    term (M 2^-76 max|x| in all: 2^-23 of one float64 rounding of the M-term sum) and 2^-63 relative in putting the limbs
    together.  x is cut into limbs as wide_kernelshap_ref.exact_sums cuts it - integers of at most 2^b in units of the grids
    g, g 2^-b, ... - with b = 52 - ceil(log2 M), so that a float64 product of 0/1 rows with such integers over M rows stays below
    2^53 and is exact in any order."""
    x = np.asarray(x, dtype=L)
    out = np.zeros((za.shape[1], zb.shape[1]), dtype=L)
    top = np.abs(x).max() if len(x) else 0
    if not top > 0:
        return out
    b = 52 - max(len(x) - 1, 1).bit_length()
    assert b >= 20
    g = L(2.0) ** (int(np.frexp(top)[1]) - b)
    rest = x.copy()
    for _ in range(-(-BITS // b)):
        if not rest.any():
            break
        p = np.round(rest / g)
        out += (za.T @ (p.astype(np.float64)[:, None] * zb)).astype(L) * g
        rest = rest - p * g
        g = g * L(2.0) ** -b
    return out


def pairs(keep, v, v0, delta, r, weights=None):
    """I (R,R) float64 of one game by the defining formula: the rows holding both of a pair weigh mu(s,2), one of them mu(s,1),
    none mu(s,0); zero diagonal."""
    z = rows_of(keep, r)
    zf = z.astype(np.float64)
    zc = 1.0 - zf
    w, d = terms(v, v0, weights, len(z))
    table = _as_long(mu(r))
    m = table[z.sum(axis=1, dtype=np.int64)]                       # (M,3): mu(s_m, .)
    x = d.astype(L)[:, None] * m
    one = pair_sums(zf, zc, x[:, 1])
    total = pair_sums(zf, zf, x[:, 2]) + (one + one.T) + pair_sums(zc, zc, x[:, 0])
    out = (L(float(delta)) / L(r - 1) + total / w.astype(L).sum()).astype(np.float64)
    np.fill_diagonal(out, 0.0)
    return out


def pairs_by_coefficients(keep, v, v0, delta, r, weights=None):
    """The same I through the alpha/beta/gamma form, every sum exact: what the identity mu = alpha + beta k + gamma [k = 2] is
    held against (CPU test; the library's form with no rounding of its own)."""
    z = rows_of(keep, r)
    zf = z.astype(np.float64)
    w, d = terms(v, v0, weights, len(z))
    c = _as_long(coefficients(r))[z.sum(axis=1, dtype=np.int64)]
    x = d.astype(L)[:, None] * c
    ones = np.ones((len(z), 1))
    a = pair_sums(ones, ones, x[:, 0])[0, 0]
    lin = pair_sums(zf, ones, x[:, 1])[:, 0]
    total = a + lin[:, None] + lin[None, :] + pair_sums(zf, zf, x[:, 2])
    out = (L(float(delta)) / L(r - 1) + total / w.astype(L).sum()).astype(np.float64)
    np.fill_diagonal(out, 0.0)
    return out


def bound(keep, v, v0, r, weights=None):
    """(M + 16) 2^-53 sum_m |d_m| (|alpha_s| + 2 |beta_s| + |gamma_s|) / W_sum: the worst case of the alpha/beta/gamma form in
    float64 under ANY summation order (each of A + L_i + L_j + Q_ij is a sum of at most M terms, their absolute values add up to
    the bracket), the 16 for the rounding of the coefficient table, of d_m and of the assembly.  Derived, not measured."""
    z = rows_of(keep, r)
    w, d = terms(v, v0, weights, len(z))
    c = np.abs(_as_float(coefficients(r)))[z.sum(axis=1, dtype=np.int64)]
    return (len(z) + 16) * U * float(np.sum(np.abs(d) * (c[:, 0] + 2 * c[:, 1] + c[:, 2]))) / float(np.sum(w))


def size_law_rows(r, count, rng, paired=True):
    """``count`` random rows of the estimator's law (size by p(s) ~ 1 / (s (R - s)), a uniform subset of that size; paired: each
    followed by its complement) -> (M,W) uint64."""
    sizes = wide.sizes_from_uniforms(r, rng.random_sample(count))
    order = np.argsort(rng.random_sample((count, r)), axis=1)
    z = np.zeros((count, r), dtype=np.uint8)
    np.put_along_axis(z, order, (np.arange(r)[None] < sizes[:, None]).astype(np.uint8), axis=1)
    if paired:
        z = np.stack([z, 1 - z], axis=1).reshape(2 * count, r)
    padded = np.zeros((len(z), 64 * wide.words(r)), dtype=np.uint8)
    padded[:, :r] = z
    return np.ascontiguousarray(np.packbits(padded, axis=1, bitorder="little")).view("<u8").astype(np.uint64)


def edge_rows(r):
    """Hand-made rows of sizes 1, 2, R-2, R-1, 0 and R (those that exist at this R) -> (k,W) uint64."""
    ids = [np.arange(s) for s in sorted({1, 2, max(r - 2, 0), r - 1, 0, r})] + [np.arange(r - 1, r), np.arange(max(r - 2, 0), r)]
    return np.array([wide.hip_ops.region_words(i, r) for i in ids], dtype=np.uint64).reshape(len(ids), wide.words(r))


def exact_sii(v, n):
    """(n,n) float64: the mean over the orders m = 0 .. n-2 of exact_ref.interactions' context-averaged I_ij^(m)."""
    import exact_ref
    pr = [(i, j) for i in range(n) for j in range(i + 1, n)]
    mean = exact_ref.interactions(v, n, pr).mean(axis=1)
    out = np.zeros((n, n))
    for (i, j), x in zip(pr, mean):
        out[i, j] = out[j, i] = x
    return out
