"""NumPy restatement of the sparse regression control variate (include/iq.h, "Sparse regression control variate"),
from the contract: the features of a pair list as products of the rows' bits, the Gram matrix as integer counts, the fit as
NumPy's float64 solve of the bordered (KKT) system, the surrogate as a longdouble product, and SHAP-IQ on the residual terms
through tests/kshap_paircv_ref.py - whose rules (folds, terms, the average, the standard error) are the same and are imported,
not restated twice.  It shares no code with interpret_quality_amd.

And a SPARSE GAME GENERATOR: a sum of unanimity games c_T u_T on sets T of 1 .. 5 regions, v(S) = base + sum_{T subset of S} c_T.
Its pairwise Shapley interaction index has the closed form I_ij = sum_{T holding i and j} c_T / (|T| - 1), and it is evaluated on
any row at any region count without a value table."""
import numpy as np

import kshap_paircv_ref as ref
import kshap_pairs_ref as pairs_ref

L = np.longdouble
MAX_FEATURES = 2080


def check_list(pairs, r):
    """The contract of a pair list -> (K,2) int64; AssertionError outside it."""
    p = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    assert r + len(p) <= MAX_FEATURES
    assert all(0 <= i < j < r for i, j in p)
    assert all(tuple(a) < tuple(b) for a, b in zip(p[:-1], p[1:]))       # strictly increasing row-major
    return p


def complete_list(r):
    """Every pair (i < j) in row-major order: the list under which the sparse surrogate is the complete one."""
    return np.array([(i, j) for i in range(r) for j in range(i + 1, r)], dtype=np.int32).reshape(-1, 2)


def expand(keep, pairs, r):
    """keep (M,) or (M,W) uint64 -> (M, r + K) uint8: the singles, then f = z_i z_j of every listed pair in list order."""
    p = check_list(pairs, r)
    z = pairs_ref.rows_of(np.asarray(keep).reshape(len(keep), -1), r)
    return np.concatenate([z, z[:, p[:, 0]] & z[:, p[:, 1]]], axis=1)


def pack(feat):
    """(M,d) uint8 feature matrix -> (M, ceil(d / 64)) uint64 feature rows, bit (a & 63) of word (a >> 6) = column a."""
    m, d = feat.shape
    padded = np.zeros((m, 64 * ((d + 63) // 64)), dtype=np.uint8)
    padded[:, :d] = feat
    return np.ascontiguousarray(np.packbits(padded, axis=1, bitorder="little")).view("<u8").astype(np.uint64)


def gram(feat):
    """(d,d) int64 counts of a (M,d) 0/1 matrix (a float64 product of integers below 2^53: exact in any order)."""
    f = np.asarray(feat).astype(np.float64)
    out = f.T @ f
    assert out.max(initial=0.0) < 2.0 ** 53
    return out.astype(np.int64)


def rhs(feat, v, v0):
    """(d,) longdouble: sum_m f_a(S_m) ((double)v_m - v0) of one game."""
    return np.asarray(feat).astype(L).T @ (np.asarray(v).astype(np.float64) - float(v0)).astype(L)


def fit(feat, v, v0, delta, ridge):
    """beta (d,) float64 of one game from the bordered system [[A, 1], [1^T, 0]] [beta; lambda] = [c; delta]."""
    d = feat.shape[1]
    k = np.zeros((d + 1, d + 1))
    k[:d, :d] = gram(feat).astype(np.float64) + float(ridge) * np.eye(d)
    k[:d, d] = k[d, :d] = 1.0
    return np.linalg.solve(k, np.concatenate([rhs(feat, v, v0).astype(np.float64), [float(delta)]]))[:d]


def surrogate(feat, beta):
    """(M,) longdouble: g_beta(S_m)."""
    return np.asarray(feat).astype(L) @ np.asarray(beta, dtype=np.float64).astype(L)


def pair_map(beta, r, pairs):
    """C(beta) (r,r): beta_{r+k} at (i_k, j_k) and (j_k, i_k), 0 elsewhere."""
    out = np.zeros((r, r))
    for k, (i, j) in enumerate(np.asarray(pairs).reshape(-1, 2)):
        out[i, j] = out[j, i] = beta[r + k]
    return out


def with_surrogate(keep, v, v0, delta, beta, r, pairs, weights=None):
    """C(beta) + (delta - sum(beta)) / (r-1) + SHAPIQ(v - v0 - g_beta) for ANY beta -> ((r,r), terms): kshap_paircv_ref's rule on
    the features of the list."""
    feat = expand(keep, pairs, r)
    t = ((np.asarray(v).astype(np.float64) - float(v0)).astype(L) - surrogate(feat, beta)).astype(np.float64)
    out = pair_map(beta, r, pairs) + ref.shapiq(keep, t, r, weights)
    slack = float((L(float(delta)) - np.asarray(beta, dtype=np.float64).astype(L).sum()) / L(r - 1))
    out[~np.eye(r, dtype=bool)] += slack
    return out, t


def pairs_cv(keep, v, v0, delta, r, pairs, paired=True, ridge=None, control="sparse"):
    """-> (I (r,r), se (r,r), betas (2,d)) float64 of one game by the contract: kshap_paircv_ref.pairs_cv with the features of
    the list; ``control="shift"`` is that module's."""
    keep = np.asarray(keep).reshape(len(keep), -1)
    v = np.asarray(v)
    if control != "sparse":
        return ref.pairs_cv(keep, v, v0, delta, r, paired, control, ridge) + (None,)
    cuts = ref.fold_rows(len(keep), paired)
    beta = [fit(expand(keep[lo:hi], pairs, r), v[lo:hi], v0, delta, (hi - lo) / 64.0 if ridge is None else ridge) for lo, hi in cuts]
    est, var, rows = [], [], []
    for f, (lo, hi) in enumerate(cuts):
        i_f, t = with_surrogate(keep[lo:hi], v[lo:hi], v0, delta, beta[1 - f], r, pairs)
        est.append(i_f)
        var.append(ref.shapiq_var(keep[lo:hi], t, r, paired))
        rows.append(hi - lo)
    m = float(rows[0] + rows[1])
    out = (rows[0] * est[0] + rows[1] * est[1]) / m
    return out, np.sqrt(np.maximum(rows[0] ** 2 * var[0] + rows[1] ** 2 * var[1], 0.0)) / m, np.stack(beta)


def neighbour_pairs(centres, k):
    """The k pairs (i < j) of smallest squared float64 distance, ties to the lexicographically smaller pair, sorted row-major -
    by a plain sort of (distance, i, j) tuples."""
    c = np.asarray(centres, dtype=np.float64)
    every = sorted((float(((c[i] - c[j]) * (c[i] - c[j])).sum()), i, j) for i in range(len(c)) for j in range(i + 1, len(c)))
    return np.array(sorted((i, j) for _, i, j in every[:k]), dtype=np.int32).reshape(-1, 2)


class SparseGame:
    """v(S) = base + sum_{T subset of S} c_T over ``sets`` (tuples of 1 .. 5 distinct regions below r) with coefficients ``coef``."""

    def __init__(self, r, sets, coef, base=0.0):
        self.r, self.base = int(r), float(base)
        self.sets = [tuple(sorted(int(i) for i in t)) for t in sets]
        self.coef = np.asarray(coef, dtype=np.float64)
        assert len(self.sets) == len(self.coef) and len(set(self.sets)) == len(self.sets)
        assert all(1 <= len(t) <= 5 and len(set(t)) == len(t) and 0 <= t[0] and t[-1] < self.r for t in self.sets)

    def values(self, keep):
        """keep (M,) or (M,W) uint64 rows -> (M,) float64 v(S_m) (sums of products of 0/1 bits with the coefficients, in list
        order: exact for integer coefficients)."""
        z = pairs_ref.rows_of(np.asarray(keep).reshape(len(keep), -1), self.r).astype(np.float64)
        out = np.full(len(z), self.base)
        for t, c in zip(self.sets, self.coef):
            out += c * np.prod(z[:, list(t)], axis=1)
        return out

    def table(self):
        """(2^r,) float64 value table (small r)."""
        masks = np.arange(1 << self.r, dtype=np.uint64)
        return self.values(masks)

    @property
    def v_empty(self):
        return self.base

    @property
    def v_full(self):
        return self.base + float(self.coef.sum())

    def index(self):
        """(r,r) float64: I_ij = sum_{T holding i and j} c_T / (|T| - 1), the closed form; zero diagonal."""
        out = np.zeros((self.r, self.r))
        for t, c in zip(self.sets, self.coef):
            for a in range(len(t)):
                for b in range(a + 1, len(t)):
                    out[t[a], t[b]] += c / (len(t) - 1)
                    out[t[b], t[a]] += c / (len(t) - 1)
        return out


def random_game(r, rng, counts=(None, 6, 5, 4, 3), integer=True):
    """A SparseGame on r regions: every single (counts[0] None) or that many, and counts[k-1] random sets of size k = 2 .. 5 (fewer
    where r has fewer), coefficients small integers or normal."""
    sets = [(i,) for i in range(r)] if counts[0] is None else []
    for size, want in enumerate(counts, start=1):
        if (size == 1 and want is None) or size > r:
            continue
        seen = set()
        while len(seen) < min(want, 50) and len(seen) < _comb(r, size):
            seen.add(tuple(sorted(rng.choice(r, size=size, replace=False).tolist())))
        sets += sorted(seen)
    coef = rng.randint(-6, 7, size=len(sets)).astype(np.float64) if integer else rng.standard_normal(len(sets))
    return SparseGame(r, sets, coef, base=3.0 if integer else float(rng.standard_normal()))


def _comb(n, k):
    from math import comb
    return comb(n, k)


CALIBRATION = {"regions": 130, "listed": 390, "unlisted": 60, "triples": 40, "units": 2000}


def calibration_game(seed=2024):
    """The game of the one statistical test -> (SparseGame, listed pairs (390,2) int32): 130 singles, the 390 neighbour pairs of a
    seeded random cloud of centres (uniform in the unit cube), 60 pairs outside that list and 40 triples, every coefficient a
    seeded standard normal."""
    rng = np.random.RandomState(seed)
    r = CALIBRATION["regions"]
    listed = neighbour_pairs(rng.random_sample((r, 3)), CALIBRATION["listed"])
    have = {tuple(p) for p in listed.tolist()}
    extra = set()
    while len(extra) < CALIBRATION["unlisted"]:
        t = tuple(sorted(rng.choice(r, size=2, replace=False).tolist()))
        if t not in have:
            extra.add(t)
    triples = set()
    while len(triples) < CALIBRATION["triples"]:
        triples.add(tuple(sorted(rng.choice(r, size=3, replace=False).tolist())))
    sets = [(i,) for i in range(r)] + [tuple(p) for p in listed.tolist()] + sorted(extra) + sorted(triples)
    return SparseGame(r, sets, rng.standard_normal(len(sets)), base=float(rng.standard_normal())), listed


def calibration_rows(seed):
    """The rows of draw ``seed``: 2000 paired units of the size law -> (4000, 3) uint64."""
    return pairs_ref.size_law_rows(CALIBRATION["regions"], CALIBRATION["units"], np.random.RandomState(seed))


def calibration_figures(out, se, se_shift, game):
    """-> (pooled z_rms over the 8385 pairs against the closed form, mean se / mean se of the shift)."""
    upper = np.triu_indices(game.r, 1)
    z = float(np.sqrt(np.mean(((out - game.index())[upper] / se[upper]) ** 2)))
    return z, float(se[upper].mean() / se_shift[upper].mean())
