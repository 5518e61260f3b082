"""NumPy / float64 brute force for the exact-game reductions, straight from the definitions in include/iq.h: loops over
subsets, no cleverness.  v is a (2^n,) float32 table, bit k of the index = player k present.  Differences are taken in
float32 exactly as the kernels (and the reference's tools/final_common.py:93, final_cal_interactions.py:33) take them; sums are
math.fsum (correctly rounded), so these values carry about one rounding of their own.

Each function can also return, per output, (t, sum|terms|): the number of terms and the sum of their magnitudes - the float64
bound for a sum of t terms in ANY order is t * 2^-53 * sum|terms|."""
import itertools
import math

import numpy as np

U = 2.0 ** -53


def popcount(c):
    return bin(int(c)).count("1")


def marginal(v, c, k):
    return float(np.float32(v[c | (1 << k)]) - np.float32(v[c]))


def interaction_term(v, c, i, j):
    bi, bj = 1 << i, 1 << j
    f = np.float32
    return float(((f(v[c | bi | bj]) + f(v[c])) - f(v[c | bi])) - f(v[c | bj]))


def shapley(v, n, with_bound=False):
    """phi[k] = sum_s w(s) * sum over {c without k, |c| = s} of (v[c + k] - v[c]), w(s) = 1 / (n C(n-1, s))."""
    phi, bound = np.zeros(n), np.zeros(n)
    for k in range(n):
        strata = [[] for _ in range(n)]
        for c in range(1 << n):
            if not (c >> k) & 1:
                strata[popcount(c)].append(marginal(v, c, k))
        phi[k] = math.fsum(math.fsum(d) / (n * math.comb(n - 1, s)) for s, d in enumerate(strata))
        bound[k] = (1 << (n - 1)) * U * math.fsum(math.fsum(abs(x) for x in d) / (n * math.comb(n - 1, s)) for s, d in enumerate(strata))
    return (phi, bound) if with_bound else phi


def interactions(v, n, pairs, with_bound=False):
    """out[p][m] = mean over the contexts c (without i, j; |c| = m) of ((v[c+i+j] + v[c]) - v[c+i]) - v[c+j]."""
    out, bound = np.zeros((len(pairs), max(n - 1, 0))), np.zeros((len(pairs), max(n - 1, 0)))
    for p, (i, j) in enumerate(pairs):
        strata = [[] for _ in range(n - 1)]
        for c in range(1 << n):
            if not (c >> i) & 1 and not (c >> j) & 1:
                strata[popcount(c)].append(interaction_term(v, c, i, j))
        for m, d in enumerate(strata):
            cnt = math.comb(n - 2, m)
            assert len(d) == cnt
            out[p, m] = math.fsum(d) / cnt
            bound[p, m] = cnt * U * math.fsum(abs(x) for x in d) / cnt
    return (out, bound) if with_bound else out


def dividends(v, n, with_bound=False):
    """a[c] = sum over subsets t of c of (-1)^(|c| - |t|) v[t]."""
    a, bound = np.zeros(1 << n), np.zeros(1 << n)
    for c in range(1 << n):
        terms = []
        t = c
        while True:      # all subsets of c
            terms.append(float(v[t]) * (-1.0) ** (popcount(c) - popcount(t)))
            if t == 0:
                break
            t = (t - 1) & c
        a[c] = math.fsum(terms)
        bound[c] = len(terms) * U * math.fsum(abs(x) for x in terms)
    return (a, bound) if with_bound else a


def shapley_from_dividends(a, n):
    """phi_k = sum over {c containing k} of a[c] / |c|."""
    return np.array([math.fsum(a[c] / popcount(c) for c in range(1, 1 << n) if (c >> k) & 1) for k in range(n)])


def interaction_term_from_dividends(a, s, i, j):
    """The interaction term of context s (without i, j) = sum of a[t + {i, j}] over the subsets t of s."""
    terms, t = [], s
    while True:
        terms.append(a[t | (1 << i) | (1 << j)])
        if t == 0:
            break
        t = (t - 1) & s
    return math.fsum(terms)


def shapley_by_permutations(v, n):
    """Mean over ALL n! permutations of the marginal contributions (n <= 6 or so)."""
    rows = []
    for order in itertools.permutations(range(n)):
        row, c = [0.0] * n, 0
        for k in order:
            row[k] = marginal(v, c, k)
            c |= 1 << k
        rows.append(row)
    return np.array([math.fsum(r[k] for r in rows) / len(rows) for k in range(n)])


def relabel(v, n, perm):
    """The same game with player k renamed perm[k]."""
    out = np.empty_like(v)
    for c in range(1 << n):
        d = 0
        for k in range(n):
            if (c >> k) & 1:
                d |= 1 << perm[k]
        out[d] = v[c]
    return out


# ---- the same sums vectorised (n = 20: the loops above would take hours) ----

def _popcounts(n):
    pc = np.zeros(1 << n, dtype=np.int64)
    for k in range(n):
        pc += (np.arange(1 << n, dtype=np.int64) >> k) & 1
    return pc


def shapley_vectorised(v, n):
    """-> (phi, bound): per stratum np.sum of the float32 differences widened to float64, divided by n C(n-1, s)."""
    v = np.asarray(v, dtype=np.float32)
    idx, pc = np.arange(1 << n, dtype=np.int64), _popcounts(n)
    phi, bound = np.zeros(n), np.zeros(n)
    for k in range(n):
        c = idx[((idx >> k) & 1) == 0]
        d = (v[c | (1 << k)] - v[c]).astype(np.float64)
        den = n * np.array([math.comb(n - 1, s) for s in range(n)], dtype=np.float64)
        phi[k] = math.fsum(np.bincount(pc[c], weights=d, minlength=n) / den)
        bound[k] = (1 << (n - 1)) * U * math.fsum(np.bincount(pc[c], weights=np.abs(d), minlength=n) / den)
    return phi, bound


def interactions_vectorised(v, n, pairs):
    v = np.asarray(v, dtype=np.float32)
    idx, pc = np.arange(1 << n, dtype=np.int64), _popcounts(n)
    out, bound = np.zeros((len(pairs), n - 1)), np.zeros((len(pairs), n - 1))
    cnt = np.array([math.comb(n - 2, m) for m in range(n - 1)], dtype=np.float64)
    for p, (i, j) in enumerate(pairs):
        bi, bj = 1 << int(i), 1 << int(j)
        c = idx[(idx & (bi | bj)) == 0]
        d = (((v[c | bi | bj] + v[c]) - v[c | bi]) - v[c | bj]).astype(np.float64)
        out[p] = np.bincount(pc[c], weights=d, minlength=n - 1) / cnt
        bound[p] = U * np.bincount(pc[c], weights=np.abs(d), minlength=n - 1)
    return out, bound


def dividends_vectorised(v, n):
    """-> (a, bound): the butterfly in float64 (bound: the same butterfly with additions on |v|, times 2^|c| 2^-53)."""
    a, m = np.asarray(v, dtype=np.float64).copy(), np.abs(np.asarray(v, dtype=np.float64))
    for b in range(n):
        a = a.reshape(-1, 2, 1 << b)
        a[:, 1, :] -= a[:, 0, :]
        m = m.reshape(-1, 2, 1 << b)
        m[:, 1, :] += m[:, 0, :]
        a, m = a.reshape(-1), m.reshape(-1)
    return a, (2.0 ** _popcounts(n)) * U * m


# ---- the oracle's value table (CPU; the reference-side half of the end-to-end checks) ----

def oracle_setup(num_regions=8, cloud=0):
    """Synthetic cloud ``cloud`` with the oracle's own FPS regions: (data (1,N,3) CPU tensor, lbl (1,), region_id (N,) int64)."""
    import torch
    from interpret_quality_amd import synth
    from oracle import ref_cpu
    pts, y = synth.make_cloud(cloud)
    data = torch.from_numpy(pts)[None]
    fps = ref_cpu.farthest_point_sample(data, num_regions)[0].numpy()
    return data, torch.tensor([y]), np.asarray(ref_cpu.cal_region_id(data, fps)).astype(np.int64)


def oracle_value_table(family, sd, data, lbl, region_id, num_regions, batch=64):
    """v[c] = the oracle's reward of the cloud that keeps the regions of the set bits of c; every other point collapses onto
    the mean of the cloud (the masking of oracle.ref_cpu.shapley_masked_batch, one coalition per row)."""
    import torch
    import probes
    from oracle import ref_cpu
    center = torch.mean(data, dim=1).reshape(1, 1, 3)
    rid = np.asarray(region_id)
    v = np.empty(1 << num_regions, dtype=np.float32)
    for lo in range(0, 1 << num_regions, batch):
        cs = np.arange(lo, min(lo + batch, 1 << num_regions))
        keep = torch.from_numpy(((cs[:, None] >> rid[None, :]) & 1).astype(bool))[:, :, None]
        full = data.expand(len(cs), data.shape[1], 3)
        masked = torch.where(keep, full, center.expand_as(full)).clone()
        logits = torch.from_numpy(probes.oracle_logits(family, sd, masked))
        v[lo:lo + len(cs)] = ref_cpu.get_reward(logits, lbl).numpy()
    return v


def sampled_rows(v, orders):
    """Per-permutation marginal contributions read off the table: (S, n) float64, what region_sv_all.npy holds."""
    orders = np.asarray(orders)
    rows = np.zeros(orders.shape)
    for s, order in enumerate(orders):
        c = 0
        for k in order:
            rows[s, k] = marginal(v, c, int(k))
            c |= 1 << int(k)
    return rows
