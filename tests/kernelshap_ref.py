"""NumPy / float64 restatement of the regression (KernelSHAP) estimator's contract (include/iq.h), straight from
the formulas: size law, row construction from orders and sizes, moments, the constrained solve through numpy.linalg.solve on
the KKT system, the analytic Gram matrix and the enumeration weights.  It shares no code with interpret_quality_amd/kernelshap.py
and is the reference of tests/test_kernelshap_gpu.py."""
import math

import numpy as np

U = 2.0 ** -53


def size_law(n):
    """p(s), s = 1 .. n-1."""
    p = np.array([1.0 / (s * (n - s)) for s in range(1, n)])
    return p / p.sum()


def size_cdf(n):
    cdf = np.cumsum(size_law(n))
    cdf[-1] = 1.0
    return cdf


def sizes_from_uniforms(n, u):
    return np.minimum(n - 1, 1 + np.searchsorted(size_cdf(n), u, side="right"))


def host_draw(n, count):
    """The host-only half of one cloud's draw on NumPy's global generator: ``count`` sizes, then ``count`` permutations as
    final_shapley_value.py:59-72 draws them -> (sizes, orders (count,n))."""
    sizes = sizes_from_uniforms(n, np.random.random_sample(count))
    orders = np.array([np.random.permutation(n) for _ in range(count)], dtype=np.int64).reshape(count, n)
    return sizes, orders


def rows_from_orders(orders, sizes, n, paired=True):
    """-> (M,) uint64 masks: the first sizes[m] entries of orders[m]; paired: followed by the complement within n bits."""
    full = (1 << n) - 1
    out = []
    for order, s in zip(np.asarray(orders), np.asarray(sizes)):
        m = 0
        for r in order[:int(s)]:
            m |= 1 << int(r)
        out.append(m)
        if paired:
            out.append(full & ~m)
    return np.array(out, dtype=np.uint64)


def membership(keep, n):
    """(M,) masks -> (M,n) float64 rows z."""
    k = np.asarray(keep).astype(np.uint64)
    return np.stack([((k >> np.uint64(i)) & np.uint64(1)).astype(np.float64) for i in range(n)], axis=1)


def moments(keep, v, v0, n, weights=None):
    """Raw sums: A = sum w z z^T (n,n), b = sum w z ((double)v - v0) (n,), W = sum w.  Every TERM is the float64 value the
    contract names (the difference in float64 after widening, times the weight); the sums over the rows are taken in extended
    precision and rounded once, so they carry no order of their own."""
    z = membership(keep, n)
    w = np.ones(len(z)) if weights is None else np.asarray(weights, dtype=np.float64)
    d = np.asarray(v).astype(np.float64) - float(v0)          # float32 rewards are widened first
    zl = z.astype(np.longdouble)
    a = (z * w[:, None]).astype(np.longdouble).T @ zl
    b = zl.T @ (w * d).astype(np.longdouble)
    return a.astype(np.float64), b.astype(np.float64), float(w.astype(np.longdouble).sum())


def moment_bounds(keep, v, v0, n, weights=None):
    """The float64 bound of a sum of t terms in any order, t 2^-53 sum|terms|, per entry of A and b (t = the rows whose term
    is not zero by construction)."""
    z = membership(keep, n)
    w = np.ones(len(z)) if weights is None else np.abs(np.asarray(weights, dtype=np.float64))
    d = np.abs(np.asarray(v).astype(np.float64) - float(v0))
    t = len(z)
    return t * U * ((z * w[:, None]).T @ z), t * U * (z.T @ (w * d))


def kkt_solve(a, b, delta):
    """[[A, 1], [1^T, 0]] [phi; lambda] = [b; delta] -> (phi, lambda)."""
    n = len(b)
    k = np.zeros((n + 1, n + 1))
    k[:n, :n] = a
    k[:n, n] = 1.0
    k[n, :n] = 1.0
    sol = np.linalg.solve(k, np.concatenate([np.asarray(b, dtype=np.float64), [float(delta)]]))
    return sol[:n], float(sol[n])


def estimate(keep, v, v_empty, v_full, n, weights=None, gram="sampled"):
    a, b, w = moments(keep, v, v_empty, n, weights)
    a = a / w if gram == "sampled" else analytic_gram(n)
    return kkt_solve(a, b / w, float(v_full) - float(v_empty))[0]


def analytic_gram(n):
    h = math.fsum(1.0 / k for k in range(1, n))
    a = np.full((n, n), 0.5 - 1.0 / (2.0 * h))
    a[np.arange(n), np.arange(n)] = 0.5
    return a


def enumerated(n):
    """All proper coalitions 1 .. 2^n - 2 with w(S) = (n-1) / (C(n,|S|) |S| (n-|S|)) -> (keep uint64, weights)."""
    keep = np.arange(1, (1 << n) - 1, dtype=np.uint64)
    size = np.array([bin(int(c)).count("1") for c in keep])
    w = np.array([(n - 1) / (math.comb(n, int(s)) * s * (n - s)) for s in size], dtype=np.float64)
    return keep, w


def cond_analytic(n):
    """cond(A) of the analytic Gram matrix: (1/2 + (n-1) A_ij) / (1/2 - A_ij)."""
    off = analytic_gram(n)[0, 1]
    return (0.5 + (n - 1) * off) / (0.5 - off)
