"""GPU: the sparse regression control variate (include/iq.h, "Sparse regression control variate"; DESIGN.md 5k;
csrc/iq_kshap_sparsecv.hip, interpret_quality_amd/sparse_ops.py) against the NumPy restatement (tests/kshap_sparse_ref.py), kernel by
kernel and end to end.

Tolerances, derived, not measured (u = 2^-53):
  expand          none: every word of a feature row is the restatement's word.
  Gram            none: every entry is an integer count and must be that integer.
  regression      none: with the complete row-major list the estimate, its standard error and both betas are the BITS of
                  control="regression" (the same counts, the same right-hand-side order, the same fit kernels, the same chain).
  solve           ||A beta_u - c||_inf <= 8 d u (||A||_inf ||beta_u||_inf + ||c||_inf), the backward-error form of a Cholesky solve,
                  c the restatement's right-hand side, the residual in extended precision; |1 beta - delta| <= 8 d u sum|beta|.
  surrogate       (d + 8) u sum_a |beta_a|: a chain of at most d additions of terms bounded by the |beta_a|.
  end to end      a game of singles and LISTED pairs with integer coefficients at ridge 0 is fitted exactly: estimate and bar to
                  1e-9 of the largest entry; the enumeration identity to kshap_pairs_ref.bound on the device's own terms (the
                  tolerance of tests/test_kshap_paircv_gpu.py with this d); the composition against the restatement to 1e-8 of
                  scale (the fits agree to the conditioning of the ridge system: a sanity bar, as there).
  lent memory     none: the same bits whatever scratch and outputs held before, and no byte written outside them.

The one statistical test, ``test_bars_are_calibrated_and_smaller_than_the_shifts_at_130_regions``: the generator game of
kshap_sparse_ref.calibration_game (130 singles, the 390 neighbour pairs of a seeded cloud of centres, 60 unlisted pairs, 40
triples, standard normal coefficients) on kshap_sparse_ref.calibration_rows(0) (2000 paired units), K = 390 listed pairs; pooled
z_rms = RMS of (estimate - closed form) / se over the 8385 pairs, and mean se (sparse) / mean se (shift).  Band and bar were
measured ONCE with the restatement (kshap_sparse_ref.pairs_cv) on the CPU over the draw seeds 0 .. 49: the band is the observed
min .. max widened by half its width on each side, the bar the largest observed ratio x 1.25.  They check the restatement's
calibration, not the kernel's.
z_rms, the 50 values:
    0.999 1.010 1.006 1.010 0.995 1.012 0.995 0.997 1.000 1.002 1.010 1.003 1.012 1.005 1.004 1.003 1.005 0.999 0.993 0.995 1.001 1.008 0.989 0.999 0.994
    0.996 1.010 1.022 1.004 1.002 0.999 1.004 1.002 1.000 0.987 1.006 1.012 1.000 0.993 0.999 0.999 1.004 0.999 0.990 1.000 0.993 1.013 1.005 0.999 0.996
    min .. max 0.9871 .. 1.0218, band 0.9697 .. 1.0391 (mean of the 50: 1.002)
mean se (sparse) / mean se (shift), the 50 values:
    0.590 0.585 0.570 0.574 0.582 0.591 0.594 0.612 0.578 0.591 0.572 0.600 0.559 0.587 0.607 0.573 0.577 0.581 0.559 0.574 0.560 0.580 0.582 0.584 0.585
    0.586 0.595 0.592 0.608 0.606 0.584 0.596 0.595 0.598 0.603 0.595 0.604 0.602 0.584 0.616 0.600 0.592 0.597 0.553 0.582 0.581 0.565 0.602 0.588 0.573
    min .. max 0.5531 .. 0.6158, bar 0.6158 x 1.25 = 0.7698
The largest ratio is below 1: at 130 regions the sparse control beats the shift.  The same draws gave RMS errors of 0.55 .. 0.62
against an index whose RMS is 0.24: at 4000 rows the map of 130 regions is still mostly noise, and the bars say so."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import guarded_alloc as G
import kshap_paircv_ref as cv_ref
import kshap_pairs_ref as pairs_ref
import kshap_sparse_ref as ref
from interpret_quality_amd import _lib, hip_ops, kernelshap, sparse_ops, wide_kernelshap

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U53 = 2.0 ** -53
L = np.longdouble

Z_BAND = (0.9697, 1.0391)
RATIO_BAR = 0.7698


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _rows(keep, r):
    """(M,W) uint64 -> device rows: narrow (M,) up to 64 regions, wide (M,W) above."""
    keep = np.asarray(keep, dtype=np.uint64).reshape(len(keep), -1)
    return _dev(keep[:, 0].copy().view(np.int64)) if r <= 64 else hip_ops.wide_masks_to_tensor(keep, DEV)


def _bits(t):
    return t.cpu().numpy().view(np.uint64)


def _all_pairs(r):
    return min(2080 - r, r * (r - 1) // 2)


def _list(r, k, rng):
    """A pair list of k pairs that holds, where k has room, (0, r-1), a pair inside one word and a pair across the first and the
    last word of the row; the rest random."""
    must = [(0, r - 1), (0, min(1, r - 1)), (min(1, r - 2), r - 1), (max(r - 3, 0), r - 1), (min(62, r - 2), min(63, r - 1))]
    if k == r * (r - 1) // 2:
        return ref.complete_list(r)
    must = [p for p in dict.fromkeys(must) if p[0] < p[1]][:k]
    have = set(must)
    while len(have) < k:
        i, j = sorted(rng.randint(r, size=2).tolist())
        if i < j:
            have.add((i, j))
    return np.array(sorted(have), dtype=np.int32).reshape(-1, 2)


def _keep_rows(r, m, rng, junk=True):
    """m rows of the size law (the empty and the full set at the end where there is room), every bit at or above r SET."""
    keep = pairs_ref.size_law_rows(r, (m + 1) // 2, rng)[:m].copy()
    if m >= 4:
        keep[-2] = 0
        keep[-1] = hip_ops.region_words(np.arange(r), r)
    if junk and r % 64:
        keep[:, -1] |= np.uint64(0xFFFFFFFFFFFFFFFF) << np.uint64(r % 64)
    return keep


# ---- expand ----

EXPAND_CASES = sorted({(r, min(k, _all_pairs(r))) for r in (2, 63, 64, 65, 129, 1024) for k in (0, 1, max(64 - r, 0), 65, 2080)})


@pytest.mark.parametrize("r,k", EXPAND_CASES)
def test_expand_is_the_restatements_words(r, k):
    rng = np.random.RandomState(1000 * r + k)
    pairs = _list(r, k, rng)
    if k >= 1:
        assert (0, r - 1) in {tuple(p) for p in pairs.tolist()}
    for m in (1, 255, 256, 257):
        keep = _keep_rows(r, m, rng)
        want = ref.pack(ref.expand(keep, pairs, r))
        got = sparse_ops.kshap_sparse_expand(_rows(keep, r), pairs, r)
        assert got.shape == (m, (r + k + 63) // 64) and got.dtype == torch.int64
        assert np.array_equal(_bits(got), want), "R=%d K=%d M=%d: %d words differ" % (r, k, m, int((_bits(got) != want).sum()))
        assert torch.equal(got, sparse_ops.kshap_sparse_expand(_rows(keep, r), pairs, r))
    if r <= 64:                                                        # a game of at most 64 regions on wide rows of one word
        assert torch.equal(got, sparse_ops.kshap_sparse_expand(hip_ops.wide_masks_to_tensor(keep, DEV), pairs, r))


def test_expand_never_indexes_with_a_list_entry_outside_the_contract():
    """The C entry cannot see the list: an entry outside 0 <= i < j < R yields a feature that no row holds (the wrapper refuses
    such a list, so this goes to the library directly), and the features around it are what they are."""
    lib = _lib.load()
    r, m = 70, 300
    rng = np.random.RandomState(70)
    keep = _keep_rows(r, m, rng)
    good = _list(r, 6, rng)
    bad = np.array([[-1, 3], [5, 5], [9, 2], [0, 70], [2 ** 31 - 1, -2 ** 31], [1 << 20, 1 << 21]], dtype=np.int32)
    both = np.concatenate([good[:3], bad, good[3:]]).astype(np.int32)
    kt, pt = _rows(keep, r), _dev(both)
    feat = torch.zeros((m, 2), dtype=torch.int64, device=DEV)
    rc = lib.iq_kshap_sparse_expand(hip_ops._p(kt), hip_ops._p(pt), m, r, len(both), hip_ops._p(feat), hip_ops._stream())
    assert rc == 0
    want = ref.expand(keep, good, r)
    full = np.concatenate([want[:, :r + 3], np.zeros((m, len(bad)), dtype=np.uint8), want[:, r + 3:]], axis=1)
    assert np.array_equal(_bits(feat), ref.pack(full))


# ---- the Gram matrix ----

@pytest.mark.parametrize("d", [2, 32, 33, 64, 65, 128, 129])
@pytest.mark.parametrize("m", [1, 255, 256, 257, 4099])
def test_gram_is_the_integer_counts(d, m):
    """Random feature rows, dense and thin, with every bit at or above d set, which must be ignored."""
    rng = np.random.RandomState(100 * d + m)
    f = (rng.random_sample((m, d)) < rng.choice([0.1, 0.5, 0.9], size=(m, 1))).astype(np.uint8)
    words = ref.pack(f)
    if d % 64:
        words[:, -1] |= np.uint64(0xFFFFFFFFFFFFFFFF) << np.uint64(d % 64)
    ft = _dev(words.view(np.int64))
    got = sparse_ops.kshap_feat_gram(ft, d)
    assert got.shape == (d, d) and got.dtype == torch.float64
    g, want = got.cpu().numpy(), ref.gram(f).astype(np.float64)
    assert np.array_equal(g, want), "d=%d M=%d: %d entries differ" % (d, m, int((g != want).sum()))
    assert torch.equal(got, sparse_ops.kshap_feat_gram(ft, d))


def test_gram_of_2080_features_at_1024_regions():
    r, k, m = 1024, 1056, 257
    rng = np.random.RandomState(1024)
    keep, pairs = _keep_rows(r, m, rng), _list(r, k, rng)
    feat = sparse_ops.kshap_sparse_expand(_rows(keep, r), pairs, r)
    got = sparse_ops.kshap_feat_gram(feat, r + k).cpu().numpy()
    assert np.array_equal(got, ref.gram(ref.expand(keep, pairs, r)).astype(np.float64))


# ---- the bits of control="regression" ----

def _cv_inputs(r, units, paired, seed, games=3):
    rng = np.random.RandomState(seed)
    keep = pairs_ref.size_law_rows(r, units, rng, paired)
    v = (rng.standard_normal((games, len(keep))) * 3).astype(np.float32)
    return keep, v, rng.standard_normal(games), rng.standard_normal(games)


@pytest.mark.parametrize("r,paired", [(9, True), (9, False), (12, True), (12, False), (64, True)])
def test_the_complete_list_is_control_regression_bit_for_bit(r, paired):
    keep, v, v0, delta = _cv_inputs(r, 301, paired, 7 * r + paired)
    kt = _rows(keep, r)
    full = ref.complete_list(r)
    want = kernelshap.pairs_cv(kt, _dev(v), v0, v0 + delta, r, paired, "regression")
    got = kernelshap.pairs_cv(kt, _dev(v), v0, v0 + delta, r, paired, "sparse", pair_list=full)
    assert got[0].shape == (3, r, r) and got[2]["beta"].shape == (2, 3, r + len(full))
    assert np.array_equal(got[0], want[0]), "interaction"
    assert np.array_equal(got[1], want[1]), "se"
    assert np.array_equal(got[2]["beta"], want[2]["beta"]), "beta"
    assert got[2]["fold_rows"] == want[2]["fold_rows"] and got[2]["ridge"] == want[2]["ridge"] and got[2]["status"] == 0
    assert got[2]["control"] == "sparse" and got[2]["features"] == r + len(full) and np.array_equal(got[2]["pairs"], full)
    assert got[2]["pairs"].dtype == np.int32 and "pairs" not in want[2] and "features" not in want[2]
    # and kernel by kernel: the feature rows' Gram matrix and surrogate are the narrow rows'
    feat = sparse_ops.kshap_sparse_expand(kt, full, r)
    d = r + len(full)
    assert torch.equal(sparse_ops.kshap_feat_gram(feat, d), hip_ops.kshap_pair_gram(kt, r))
    beta = _dev(want[2]["beta"][0])
    a, b = sparse_ops.kshap_feat_surrogate(feat, beta, d, _dev(v), _dev(v0)), hip_ops.kshap_pair_surrogate(kt, beta, r, _dev(v), _dev(v0))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---- fit and surrogate ----

@pytest.mark.parametrize("r,k,m", [(130, 70, 600), (1024, 1056, 600)])
def test_fit_and_surrogate_to_the_derived_bounds(r, k, m):
    rng = np.random.RandomState(31 * r + k)
    keep, pairs = _keep_rows(r, m, rng), _list(r, k, rng)
    d, ridge = r + k, m / 64.0
    v = (rng.standard_normal((2, m)) * 3).astype(np.float32)
    v0, delta = rng.standard_normal(2), rng.standard_normal(2)
    feat = sparse_ops.kshap_sparse_expand(_rows(keep, r), pairs, r)
    gram = sparse_ops.kshap_feat_gram(feat, d)
    beta_t, solves_t = sparse_ops.kshap_feat_fit(gram, feat, _dev(v), _dev(v0), _dev(delta), d, ridge, solves=True)
    beta, solves = beta_t.cpu().numpy(), solves_t.cpu().numpy()
    assert beta.shape == (2, d) and solves.shape == (3, d)
    again = sparse_ops.kshap_feat_fit(gram, feat, _dev(v), _dev(v0), _dev(delta), d, ridge)
    assert torch.equal(again, beta_t), "two calls"
    one = sparse_ops.kshap_feat_fit(gram, feat, _dev(v[1:2]), _dev(v0[1:2]), _dev(delta[1:2]), d, ridge)
    assert torch.equal(one[0], beta_t[1]), "a game's bits depend on G"
    f = ref.expand(keep, pairs, r)
    a = ref.gram(f).astype(L) + L(ridge) * np.eye(d, dtype=L)
    a_norm = float(np.abs(a).sum(axis=1).max())
    rhs = [ref.rhs(f, v[g], v0[g]) for g in range(2)] + [np.ones(d, dtype=L)]
    for g in range(3):
        x = solves[g].astype(L)
        resid = float(np.abs(a @ x - rhs[g]).max())
        bound = 8 * d * U53 * (a_norm * float(np.abs(x).max()) + float(np.abs(rhs[g]).max()))
        print("R=%d K=%d rhs %d: residual %.3g, bound %.3g, fraction %.3g" % (r, k, g, resid, bound, resid / bound))
        assert resid <= bound, (r, k, g)
    for g in range(2):
        gap = abs(float(beta[g].astype(L).sum() - L(delta[g])))
        bound = 8 * d * U53 * float(np.abs(beta[g]).sum())
        print("R=%d K=%d game %d: |sum(beta) - delta| = %.3g, bound %.3g" % (r, k, g, gap, bound))
        assert gap <= bound, (r, k, g)
    out_g, out_t = sparse_ops.kshap_feat_surrogate(feat, beta_t, d, _dev(v), _dev(v0))
    assert torch.equal(out_g, sparse_ops.kshap_feat_surrogate(feat, beta_t, d))
    assert torch.equal(sparse_ops.kshap_feat_surrogate(feat, beta_t[1:2].contiguous(), d)[0], out_g[1])
    gh, th = out_g.cpu().numpy(), out_t.cpu().numpy()
    for g in range(2):
        err = float(np.abs(gh[g].astype(L) - ref.surrogate(f, beta[g])).max())
        bound = (d + 8) * U53 * float(np.abs(beta[g]).sum())
        print("R=%d K=%d game %d: surrogate error %.3g, bound %.3g" % (r, k, g, err, bound))
        assert err <= bound
        assert np.array_equal(th[g], (v[g].astype(np.float64) - v0[g]) - gh[g])          # the terms: two roundings


def test_a_singular_system_at_ridge_0_is_refused():
    z = torch.zeros((1,), dtype=torch.float64, device=DEV)
    r, pairs = 130, _list(130, 70, np.random.RandomState(3))
    for keep in (np.zeros((40, 3), dtype=np.uint64), _keep_rows(r, 40, np.random.RandomState(5))):      # a zero matrix; 40 rows, 200 unknowns
        feat = sparse_ops.kshap_sparse_expand(_rows(keep, r), pairs, r)
        gram = sparse_ops.kshap_feat_gram(feat, 200)
        v = torch.ones((1, 40), dtype=torch.float32, device=DEV)
        with pytest.raises(hip_ops.KshapSingular):
            sparse_ops.kshap_feat_fit(gram, feat, v, z, z + 1.0, 200, 0.0)
        assert sparse_ops.kshap_feat_fit(gram, feat, v, z, z + 1.0, 200, 40 / 64.0).shape == (1, 200)    # and the ridge alone mends it


# ---- exactness ----

def test_a_game_of_singles_and_listed_pairs_is_returned_exactly_at_130_regions():
    r, rng = 130, np.random.RandomState(130)
    pairs = _list(r, 70, rng)
    game = ref.SparseGame(r, [(i,) for i in range(r)] + [tuple(p) for p in pairs.tolist()], rng.randint(-5, 6, size=r + 70), base=3.0)
    keep = pairs_ref.size_law_rows(r, 1000, rng)                      # 2000 paired rows, 1000 per fold, 200 unknowns
    values = game.values(keep)
    v = values.astype(np.float32)
    assert np.array_equal(v.astype(np.float64), values)
    out, se, info = wide_kernelshap.pairs_cv(_rows(keep, r), _dev(v), game.v_empty, game.v_full, r, control="sparse", ridge=0.0,
                                             pair_list=pairs)
    want = game.index()
    top = np.abs(want).max()
    print("listed game: max error %.3g, max se %.3g, largest entry %g" % (np.abs(out - want).max(), se.max(), top))
    assert out.shape == se.shape == (r, r) and np.array_equal(want, kernelshap.sparse_coefficient_map(game.coef, r, pairs))
    assert np.abs(out - want).max() <= 1e-9 * top and se.max() <= 1e-9 * top
    assert info["fold_rows"] == [1000, 1000] and info["ridge"] == [0.0, 0.0] and info["status"] == 0 and info["beta"].shape == (2, 200)
    assert np.abs(info["beta"] - game.coef[None]).max() <= 1e-9 * np.abs(game.coef).max()


@pytest.mark.parametrize("n", range(2, 11))
def test_enumerated_rows_and_any_beta_on_a_sparse_list_give_the_exact_index(n):
    rng = np.random.RandomState(60 + n)
    v = np.random.default_rng(720 + n).integers(-40, 41, size=1 << n).astype(np.float32)
    full = ref.complete_list(n)
    pairs = full[np.sort(rng.choice(len(full), size=(len(full) + 1) // 2, replace=False))]
    d = n + len(pairs)
    delta = float(v[-1]) - float(v[0])
    beta = rng.standard_normal((2, d)) * 10.0
    beta[1] *= 1e6
    keep, weights = kernelshap.enumerated(n, DEV)
    rows = keep.cpu().numpy().view(np.uint64).reshape(-1, 1)
    vt = _dev(v).index_select(0, keep).reshape(1, -1).expand(2, -1).contiguous()
    v0t = torch.full((2,), float(v[0]), dtype=torch.float64, device=DEV)
    feat = sparse_ops.kshap_sparse_expand(keep, pairs, n)
    _, t = sparse_ops.kshap_feat_surrogate(feat, _dev(beta), d, vt, v0t)
    res = hip_ops.kshap_pairs_terms(keep, t, n, weights).cpu().numpy()
    want = pairs_ref.exact_sii(v, n)
    th, wh = t.cpu().numpy(), weights.cpu().numpy()
    off = ~np.eye(n, dtype=bool)
    weight_of_a_term = cv_ref.bound(rows, np.ones(len(rows)), n, wh) / ((len(rows) + 16) * U53)
    for g in range(2):
        got = kernelshap.sparse_coefficient_map(beta[g], n, pairs) + res[g] + np.where(off, (delta - beta[g].sum()) / (n - 1), 0.0)
        tol = (cv_ref.bound(rows, th[g], n, wh) + (d + 8) * U53 * np.abs(beta[g]).sum() * weight_of_a_term
               + (d + 8) * U53 * (np.abs(beta[g]).sum() + abs(delta)))
        err = np.abs(got - want).max()
        print("n=%d K=%d beta %d: error %.3g, tolerance %.3g" % (n, len(pairs), g, err, tol))
        assert err <= tol


# ---- the bits of pairs_cv ----

@pytest.mark.parametrize("r,k", [(12, 5), (65, 0), (130, 200)])
@pytest.mark.parametrize("paired", [True, False])
def test_bits_of_pairs_cv(r, k, paired):
    keep, v, v0, delta = _cv_inputs(r, 301, paired, 11 * r + paired)
    pairs = _list(r, k, np.random.RandomState(r + k))
    kt = _rows(keep, r)
    ks = wide_kernelshap if r > 64 else kernelshap
    out, se, info = ks.pairs_cv(kt, _dev(v), v0, v0 + delta, r, paired, "sparse", pair_list=pairs)
    assert out.shape == se.shape == (3, r, r) and out.dtype == se.dtype == np.float64
    for x in (out, se):
        assert np.array_equal(x, x.transpose(0, 2, 1)) and not np.diagonal(x, axis1=1, axis2=2).any() and np.isfinite(x).all()
    again = ks.pairs_cv(kt, _dev(v), v0, v0 + delta, r, paired, "sparse", pair_list=pairs.tolist())
    assert np.array_equal(out, again[0]) and np.array_equal(se, again[1]) and np.array_equal(info["beta"], again[2]["beta"]), "two calls"
    c = 2 if paired else 1
    assert info["fold_rows"] == [c * 150, c * 151] and info["ridge"] == [c * 150 / 64.0, c * 151 / 64.0]
    assert info["beta"].shape == (2, 3, r + k) and info["features"] == r + k and np.array_equal(info["pairs"], pairs)
    for g in range(3):                                                # a game's bits depend neither on G nor on its place
        o1, s1, i1 = ks.pairs_cv(kt, _dev(v[g]), v0[g], v0[g] + delta[g], r, paired, "sparse", pair_list=pairs)
        assert o1.shape == (r, r) and np.array_equal(o1, out[g]) and np.array_equal(s1, se[g]), g
        assert np.array_equal(i1["beta"], info["beta"][:, g])
    poisoned = v.copy()
    poisoned[1] = np.nan                                              # the games never meet
    o2, s2, _ = ks.pairs_cv(kt, _dev(poisoned), v0, v0 + delta, r, paired, "sparse", pair_list=pairs)
    assert np.array_equal(o2[0], out[0]) and np.array_equal(o2[2], out[2]) and np.array_equal(s2[0], se[0]) and np.array_equal(s2[2], se[2])
    assert np.isnan(o2[1]).any()
    want, want_se, _ = ref.pairs_cv(keep, v[0], v0[0], delta[0], r, pairs, paired)
    scale = np.abs(want).max()
    print("R=%d K=%d: against the restatement %.3g and %.3g of scale" % (r, k, np.abs(out[0] - want).max() / scale,
                                                                        np.abs(se[0] - want_se).max() / scale))
    assert np.abs(out[0] - want).max() <= 1e-8 * scale and np.abs(se[0] - want_se).max() <= 1e-8 * scale


# ---- calibration and gain ----

def test_bars_are_calibrated_and_smaller_than_the_shifts_at_130_regions():
    game, listed = ref.calibration_game()
    r = game.r
    assert r == 130 and listed.shape == (390, 2) and len(game.sets) == 130 + 390 + 60 + 40
    assert np.array_equal(listed, kernelshap.neighbour_pairs(np.random.RandomState(2024).random_sample((r, 3)), 390))
    keep = ref.calibration_rows(0)
    assert keep.shape == (4000, 3)
    v = game.values(keep).astype(np.float32)
    v_empty, v_full = float(np.float32(game.v_empty)), float(np.float32(game.v_full))
    kt, vt = _rows(keep, r), _dev(v)
    out, se, info = wide_kernelshap.pairs_cv(kt, vt, v_empty, v_full, r, True, "sparse", pair_list=listed)
    _, se_shift, _ = wide_kernelshap.pairs_cv(kt, vt, v_empty, v_full, r, True, "shift")
    z, ratio = ref.calibration_figures(out, se, se_shift, game)
    upper = np.triu_indices(r, 1)
    print("sparse, K = 390: z_rms %.4f (band %s), mean se / mean se of the shift %.4f (at most %g), rms error %.4g, index rms %.4g" % (
        z, Z_BAND, ratio, RATIO_BAR, float(np.sqrt(np.mean((out - game.index())[upper] ** 2))),
        float(np.sqrt(np.mean(game.index()[upper] ** 2)))))
    assert info["features"] == 520 and info["fold_rows"] == [2000, 2000]
    assert Z_BAND[0] <= z <= Z_BAND[1]
    assert ratio <= RATIO_BAR


# ---- lent memory: exact sizes, guard zones, hostile prior contents ----

class _LentMemory(G.TorchProxy):
    """tests/guarded_alloc.py's proxy for wrappers that allocate with ``torch.zeros``: every float64 device buffer they make -
    scratch and outputs, the memory the library is LENT - and the int64 feature rows that ``kshap_sparse_expand`` is lent become a
    Guarded body of exactly its size with the fill's hostile contents; the int32 status word stays the zeroed word the contract
    asks the caller for."""

    def zeros(self, *size, **kw):
        if kw.get("dtype") in (torch.float64, torch.int64) and kw.get("device") is not None:
            return self.empty(*size, **kw)
        return torch.zeros(*size, **kw)


def _lent(fill, fn):
    """``fn`` with sparse_ops' module global ``torch`` replaced -> (its tensors, the Recording); every guard is checked."""
    rec = G.Recording()
    assert sparse_ops.torch is torch
    sparse_ops.torch = _LentMemory(fill, rec, "cuda")
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        sparse_ops.torch = torch
    rec.check()
    if isinstance(fill, G.STALE):
        fill.finish()
    return [t for t in (out if isinstance(out, (tuple, list)) else [out]) if isinstance(t, torch.Tensor)], rec


def _lent_op(kind, r, k, seed):
    rng = np.random.RandomState(1000 * seed + r)
    keep = pairs_ref.size_law_rows(r, 40, rng)
    pairs = _list(r, k, np.random.RandomState(r))
    kt = _rows(keep, r)
    m, d = len(keep), r + k
    v, v0, delta = _dev((rng.standard_normal((3, m)) * 3).astype(np.float32)), _dev(rng.standard_normal(3)), _dev(rng.standard_normal(3))
    if kind == "kshap_sparse_expand":
        return lambda: sparse_ops.kshap_sparse_expand(kt, pairs, r)
    feat = sparse_ops.kshap_sparse_expand(kt, pairs, r)
    if kind == "kshap_feat_gram":
        return lambda: sparse_ops.kshap_feat_gram(feat, d)
    if kind == "kshap_feat_fit":
        gram = sparse_ops.kshap_feat_gram(feat, d)
        return lambda: sparse_ops.kshap_feat_fit(gram, feat, v, v0, delta, d, 1.0, solves=True)
    beta = _dev(rng.standard_normal((3, d)))
    return lambda: sparse_ops.kshap_feat_surrogate(feat, beta, d, v, v0)


# 17 features: one panel of the factor, one block; 200: seven panels, ten blocks of the Gram matrix, wide rows
LENT = [(kind, r, k) for kind in ("kshap_sparse_expand", "kshap_feat_gram", "kshap_feat_fit", "kshap_feat_surrogate")
        for r, k in ((12, 5), (130, 70))]


def _same_bits(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and torch.equal(
        x.contiguous().reshape(-1).view(torch.uint8), y.contiguous().reshape(-1).view(torch.uint8)) for x, y in zip(a, b))


@pytest.mark.parametrize("kind,r,k", LENT)
def test_results_do_not_depend_on_what_the_lent_memory_held(kind, r, k):
    """The plain result again when the float64 scratch and outputs are exactly as large as asked, stand between guard zones, and
    held zeros, 0xFF bytes (every float64 a NaN) or the bytes another call on the same shape left: nothing is read before it is
    written and nothing is written outside (for ``kshap_sparse_expand`` the lent memory is its int64 feature rows)."""
    fn, donor_fn = _lent_op(kind, r, k, 0), _lent_op(kind, r, k, 1)
    out = fn()
    plain = [t for t in (out if isinstance(out, (tuple, list)) else [out])]
    torch.cuda.synchronize()
    for name, fill in (("ZERO", G.ZERO), ("ONES", G.ONES)):
        got, rec = _lent(fill, fn)
        assert len(rec) >= 1 and _same_bits(got, plain), "%s: the result under %s is not the plain result" % (kind, name)
    _, donor = _lent(G.ZERO, donor_fn)
    got, rec = _lent(G.STALE(donor), fn)
    assert rec.sizes() == donor.sizes() and _same_bits(got, plain), "%s: the result on a donor's bytes is not the plain result" % kind


# ---- refusals on the device ----

def test_refusals():
    keep = torch.ones((8,), dtype=torch.int64, device=DEV)
    v = torch.zeros((1, 8), dtype=torch.float32, device=DEV)
    wide = torch.ones((8, 2), dtype=torch.int64, device=DEV)
    for pairs in ([[0, 2], [0, 1]], [[0, 1], [0, 1]], [[1, 1]], [[0, 8]]):
        with pytest.raises(_lib.IqError):
            kernelshap.pairs_cv(keep, v, 0.0, 1.0, 8, control="sparse", pair_list=pairs)
    with pytest.raises(_lib.IqError, match="shift"):
        kernelshap.pairs_cv(wide, v, 0.0, 1.0, 65, control="regression")                     # still refused, still names the shift
    out, se, info = kernelshap.pairs_cv(wide, v, 0.0, 1.0, 65, control="sparse", pair_list=[])
    assert out.shape == (1, 65, 65) and info["features"] == 65 and info["pairs"].shape == (0, 2)
    with pytest.raises(_lib.IqError, match="feat must be"):
        sparse_ops.kshap_feat_gram(wide, 200)
    with pytest.raises(_lib.IqError, match="ridge"):
        sparse_ops.kshap_feat_fit(torch.zeros((9, 9), dtype=torch.float64, device=DEV), keep.reshape(8, 1), v,
                                  torch.zeros((1,), dtype=torch.float64, device=DEV), torch.zeros((1,), dtype=torch.float64, device=DEV), 9, -1.0)


# ---- drivers ----

def _run(script, cwd, extra):
    env = dict(os.environ, PYTHONPATH=REPO)
    cmd = [sys.executable, os.path.join(REPO, script), "--model", "pointnet", "--dataset", "modelnet10", "--synthetic", "--num_clouds", "1"] + extra
    r = subprocess.run(cmd, cwd=str(cwd), env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


NEW_FILES = ["region_interaction_cv.npy", "region_interaction_cv_se.npy", "control.json", "control_pairs.npy"]


def _check_driver(tmp_path, script, n, samples, k, extra):
    """One child with --control sparse, one without: the flag adds the four files and changes no other byte."""
    flags = ["--num_regions", str(n), "--samples", str(samples), "--pairs"]
    (tmp_path / "with").mkdir()
    (tmp_path / "without").mkdir()
    _run(script, tmp_path / "with", flags + ["--control", "sparse"] + extra)
    _run(script, tmp_path / "without", flags)
    folder = "exp_MODEL_pointnet_DATA_modelnet10_POINTNUM_1024_REGIONNUM_%d_shapley_test" % n
    a, b = (tmp_path / w / "checkpoints" / folder / "synthetic_00" / "kernelshap" for w in ("with", "without"))
    names = sorted(os.listdir(b))
    assert sorted(os.listdir(a)) == sorted(names + NEW_FILES), (sorted(os.listdir(a)), names)
    assert [x for x in names if (a / x).read_bytes() != (b / x).read_bytes()] == []
    got, se = np.load(a / "region_interaction_cv.npy"), np.load(a / "region_interaction_cv_se.npy")
    for x in (got, se):
        assert x.shape == (n, n) and x.dtype == np.float64 and np.array_equal(x, x.T) and not np.diag(x).any() and np.isfinite(x).all()
    assert (se[np.triu_indices(n, 1)] > 0).all()
    pairs = np.load(a / "control_pairs.npy")
    assert pairs.shape == (k, 2) and pairs.dtype == np.int32
    sparse_ops.check_pair_list(pairs, n)
    info = json.load(open(a / "control.json"))
    assert set(info) == {"control", "select", "pairs", "features", "fold_rows", "ridge", "status"}
    assert info["control"] == "sparse" and info["select"] == "neighbours" and info["pairs"] == k and info["features"] == n + k
    assert sum(info["fold_rows"]) == samples and info["ridge"] == [f / 64.0 for f in info["fold_rows"]] and info["status"] == 0
    return a, got, se, pairs


def test_final_kernel_shapley_with_control_sparse(tmp_path):
    _check_driver(tmp_path, "final_kernel_shapley.py", 8, 256, 5, ["--control_pairs", "5"])


def test_final_wide_kernel_shapley_with_control_sparse(tmp_path):
    _check_driver(tmp_path, "final_wide_kernel_shapley.py", 65, 400, 195, [])
