"""NumPy restatement of the wide regression (KernelSHAP) estimator's contract (include/iq.h), straight from the
formulas: the size law and the host-only draw, wide rows from orders and sizes, the moment b summed exactly and rounded once, with
the float64 bound of a sum in any order, and phi both ways - the closed form that the analytic Gram matrix allows, and a KKT solve with that matrix written
out densely.  It shares no code with interpret_quality_amd/wide_kernelshap.py (hip_ops.region_words, the host builder of wide
rows, is the one import) and is the reference of tests/test_wide_kernelshap_gpu.py."""
import math
from fractions import Fraction

import numpy as np

import kernelshap_ref as narrow
from interpret_quality_amd import hip_ops

U = 2.0 ** -53
L = np.longdouble

size_cdf = narrow.size_cdf                        # the formulas hold for any n >= 2
sizes_from_uniforms = narrow.sizes_from_uniforms
cond_analytic = narrow.cond_analytic
analytic_gram = narrow.analytic_gram
kkt_solve = narrow.kkt_solve


def host_draw(r, count):
    """The host-only draw of one cloud on NumPy's global generator: ``random_sample(count)`` -> sizes, then ``count`` times
    ``np.random.permutation(r)`` -> (sizes, orders (count,r))."""
    sizes = sizes_from_uniforms(r, np.random.random_sample(count))
    orders = np.array([np.random.permutation(r) for _ in range(count)], dtype=np.int64).reshape(count, r)
    return sizes, orders


def words(r):
    return (r + 63) // 64


def full_row(r):
    return hip_ops.region_words(np.arange(r), r)


def rows_from_orders(orders, sizes, r, paired=True):
    """-> (M,W) uint64 rows: the first sizes[m] entries of orders[m]; paired: followed by the complement within the R bits."""
    full = full_row(r)
    out = []
    for order, s in zip(np.asarray(orders), np.asarray(sizes)):
        row = hip_ops.region_words(np.asarray(order)[:int(s)], r)
        out.append(row)
        if paired:
            out.append(full & ~row)
    return np.array(out, dtype=np.uint64).reshape(-1, words(r))


def bits(keep, r):
    """(M,W) rows -> (M,R) uint8 rows z (bits at or above R are not looked at)."""
    k = np.ascontiguousarray(np.asarray(keep, dtype="<u8").reshape(-1, words(r)))
    return np.unpackbits(k.view(np.uint8), axis=1, bitorder="little")[:, :r]


def membership(keep, r):
    """(M,W) rows -> (M,R) float64 rows z."""
    return bits(keep, r).astype(np.float64)


ROWS = 8192      # rows of z held as float64 at a time (64 MB at 1024 regions)


def _column_sums(z, x):
    """z (M,R) uint8, x (M,C) float64 -> (R,C) float64 z^T x, ROWS rows at a time."""
    out = np.zeros((z.shape[1], x.shape[1]))
    for lo in range(0, len(z), ROWS):
        out += z[lo:lo + ROWS].T.astype(np.float64) @ x[lo:lo + ROWS]
    return out


def exact_sums(z, d):
    """z (M,R) uint8, d (M,C) float64 -> (C,R) float64: sum_m z[m,i] d[m,c] EXACTLY, rounded once - what math.fsum returns, for a
    million terms per entry.  Each column of d is cut into limbs on the grids g, g 2^-26, g 2^-52, ... with g = 2^(e-26) and
    max|d| < 2^e: a limb is d's remainder rounded to its grid, an integer of at most 2^26 in units of the grid, and the remainder
    after it is exact (fewer bits than d, all below the grid).  A float64 sum of up to 2^26 such integers is exact in any order, so
    the limbs go through one BLAS product; the limb sums are put together as fractions and rounded once."""
    d = np.asarray(d, dtype=np.float64).reshape(len(z), -1)
    m, c = d.shape
    assert m <= 1 << 26
    top = np.abs(d).max(axis=0)
    g = 2.0 ** (np.frexp(np.where(top > 0, top, 1.0))[1] - 26)
    limbs, grids, rest = [], [], d.copy()
    while rest.any():
        p = np.round(rest / g)
        limbs.append(p)
        grids.append(g)
        rest = rest - p * g
        g = g * 2.0 ** -26
    out = np.zeros((c, z.shape[1]))
    if limbs:
        s = _column_sums(z, np.concatenate(limbs, axis=1))
        for col in range(c):
            for i in range(z.shape[1]):
                out[col, i] = float(sum(Fraction(int(s[i, k * c + col])) * Fraction(float(grids[k][col])) for k in range(len(limbs))))
    return out


def _terms(v, v0, weights, m):
    """-> (w (M,), d (M,G)): the float64 terms the contract names - float32 rewards widened first, one rounding for the difference
    and one for the product with the weight."""
    w = np.ones(m) if weights is None else np.asarray(weights, dtype=np.float64)
    v = np.asarray(v).astype(np.float64).reshape(-1, m)
    return w, (w[None] * (v - np.asarray(v0, dtype=np.float64).reshape(-1, 1))).T


def moment(keep, v, v0, r, weights=None):
    """Raw sums b = sum w z ((double)v - v0) and W = sum w; v (M,) with a scalar v0 -> b (R,), or v (G,M) with v0 (G,) -> b (G,R).
    Every TERM is the float64 value the contract names; the sums over the rows are exact and rounded once (``exact_sums``,
    math.fsum), so they carry no order of their own."""
    z = bits(keep, r)
    w, d = _terms(v, v0, weights, len(z))
    b = exact_sums(z, d)
    return (b[0] if np.ndim(v) == 1 else b), math.fsum(w)


def moment_bound(keep, v, v0, r, weights=None):
    """The float64 bound of a sum of t terms in any order, t 2^-53 sum|terms|, per entry of b (as kernelshap_ref.moment_bounds),
    shaped like ``moment``'s b."""
    z = bits(keep, r)
    _, d = _terms(v, v0, weights, len(z))
    bound = len(z) * U * _column_sums(z, np.abs(d)).T
    return bound[0] if np.ndim(v) == 1 else bound


def harmonic(r):
    """H_{R-1}."""
    return math.fsum(1.0 / k for k in range(1, r))


def closed_form(b_raw, wsum, delta, r):
    """phi_i = 2 H_{R-1} (b_i - mean(b)) + delta / R with b = b_raw / wsum, evaluated in extended precision -> (R,) longdouble."""
    b = np.asarray(b_raw, dtype=np.float64).astype(L) / L(wsum)
    return 2 * L(harmonic(r)) * (b - b.sum() / L(r)) + L(delta) / L(r)


def kkt(b_raw, wsum, delta, r):
    """The same phi from the KKT system with the dense analytic Gram matrix (numpy.linalg.solve, float64)."""
    return kkt_solve(analytic_gram(r), np.asarray(b_raw, dtype=np.float64) / wsum, delta)[0]


def estimate(keep, v, v_empty, v_full, r, weights=None):
    b, w = moment(keep, v, v_empty, r, weights)
    return closed_form(b, w, float(v_full) - float(v_empty), r).astype(np.float64)


def enumerated(n):
    """kernelshap_ref.enumerated with the rows widened to (2^n - 2, 1)."""
    keep, w = narrow.enumerated(n)
    return keep.reshape(-1, 1), w
