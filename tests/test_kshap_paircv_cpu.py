"""CPU: the control-variate estimators of the all-pairs map (include/iq.h, "Control variates for the all-pairs map") -
the identities that make them unbiased, held on the NumPy restatement (tests/kshap_paircv_ref.py): for ANY coefficients beta the
pair coefficients plus SHAP-IQ on the residuals of the enumerated rows is the exact index, the same for the shift, and the
complement symmetry of the weights behind the shift; the restated scratch and fold sizes against the library's; and the
plumbing: the entry points declared, bound and exported at ABI 122, their argument checks, both drivers' --control flag."""
import os
import re

import numpy as np
import pytest

import kshap_paircv_ref as ref
import kshap_pairs_ref as pairs_ref
import wide_kernelshap_ref as wide_ref
from interpret_quality_amd import _lib, build, kernelshap, wide_kernelshap

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("iq_kshap_pairs_terms", "iq_kshap_pairs_terms_se", "iq_kshap_pair_features", "iq_kshap_pair_gram",
         "iq_kshap_pair_fit_scratch_bytes", "iq_kshap_pair_fit", "iq_kshap_pair_surrogate", "iq_kshap_pair_shift_terms")


def _integer_table(n, seed):
    """A float32 table of small integers: every float32 difference and every widening is exact."""
    return np.random.default_rng(seed).integers(-40, 41, size=1 << n).astype(np.float32)


def _betas(n, rng):
    d = ref.feature_count(n)
    return {"zero": np.zeros(d), "random": rng.standard_normal(d) * 10.0, "huge": rng.standard_normal(d) * 1e12,
            "one huge pair": np.concatenate([np.zeros(d - 1), [-3e15]])}


@pytest.mark.parametrize("n", range(2, 9))
def test_any_surrogate_leaves_the_enumerated_estimate_exact(n):
    """Conditional unbiasedness in its sharpest form: over the enumerated rows with enumeration_weights the estimator IS its
    expectation, so C(beta) + (delta - sum beta) / (n-1) + SHAPIQ(v - v0 - g_beta) must be the exact index for every beta,
    efficient or not, to the rounding of the residual terms: kshap_pairs_ref.bound computed on them."""
    v = _integer_table(n, 220 + n)
    keep, w = wide_ref.enumerated(n)
    rows = v[keep[:, 0].astype(np.int64)]
    delta = float(v[-1]) - float(v[0])
    want = pairs_ref.exact_sii(v, n)
    for name, beta in _betas(n, np.random.RandomState(n)).items():
        got, t = ref.with_surrogate(keep, rows, v[0], delta, beta, n, w)
        tol = ref.bound(keep, t, n, w)
        err = np.abs(got - want).max()
        print("n=%d %s: error %.3g, tolerance %.3g" % (n, name, err, tol))
        assert err <= tol, (n, name)
        assert np.array_equal(got, got.T) and not np.diag(got).any()


@pytest.mark.parametrize("n", range(2, 9))
def test_the_shift_leaves_the_enumerated_estimate_exact(n):
    v = _integer_table(n, 320 + n)
    keep, w = wide_ref.enumerated(n)
    rows = v[keep[:, 0].astype(np.int64)]
    delta = float(v[-1]) - float(v[0])
    t = ref.shift_terms(keep, rows, v[0], delta, n)
    got = ref.shapiq(keep, t, n, w)
    err = np.abs(got - pairs_ref.exact_sii(v, n)).max()
    tol = ref.bound(keep, t, n, w)
    print("n=%d: error %.3g, tolerance %.3g" % (n, err, tol))
    assert err <= tol


def test_weights_are_symmetric_under_the_complement():
    """mu(s, k) = mu(R - s, 2 - k) in exact rationals: a row and its complement weigh a pair alike, which is why an additive part of
    the game reaches a paired unit only through its total."""
    for r in range(2, 65):
        mu = pairs_ref.mu(r)
        for s in range(1, r):
            for k in range(3):
                assert mu[s, k] == mu[r - s, 2 - k], (r, s, k)


def test_restatement_of_the_fit_and_the_features():
    rng = np.random.RandomState(3)
    for r in (2, 3, 6):
        masks = ref.feature_masks(r)
        assert len(masks) == ref.feature_count(r) == kernelshap.pair_features(r) and len(set(masks)) == len(masks)
        assert masks[:r] == [1 << i for i in range(r)] and masks[r] == 3 and masks[-1] == (3 << (r - 2))
        keep = pairs_ref.size_law_rows(r, 40, rng)
        f = ref.features(keep, r)
        assert np.array_equal(f, ref.features_by_masks(keep, r))
        z = pairs_ref.rows_of(keep, r)
        assert np.array_equal(f[:, :r], z)
        assert np.array_equal(ref.gram(keep, r), f.astype(np.int64).T @ f.astype(np.int64))
        v = rng.standard_normal(len(keep)).astype(np.float32)
        beta = ref.fit(keep[:, 0], v, 0.25, 1.5, r, 0.5)
        assert abs(beta.sum() - 1.5) <= 1e-12 * max(1.0, np.abs(beta).sum())
        assert np.array_equal(kernelshap.pair_coefficient_map(beta, r), ref.pair_map(beta, r))
        assert np.array_equal(kernelshap.pair_coefficient_map(np.stack([beta, 2 * beta]), r)[1], 2 * ref.pair_map(beta, r))


def test_restatement_returns_a_two_additive_game_exactly():
    """A 2-additive integer table, ridge 0: every fold's fit is the game itself, the residuals vanish, the estimate is the exact
    index and its standard error nothing."""
    n, rng = 6, np.random.RandomState(11)
    beta = rng.randint(-5, 6, size=ref.feature_count(n)).astype(np.float64)
    masks = ref.feature_masks(n)
    table = np.array([3.0 + sum(b for b, fm in zip(beta, masks) if s & fm == fm) for s in range(1 << n)], dtype=np.float32)
    keep = pairs_ref.size_law_rows(n, 200, rng)
    v = table[keep[:, 0].astype(np.int64)]
    out, se = ref.pairs_cv(keep, v, table[0], float(table[-1]) - float(table[0]), n, ridge=0.0)
    want = pairs_ref.exact_sii(table, n)
    assert np.array_equal(want, ref.pair_map(beta, n))
    assert np.abs(out - want).max() <= 1e-9 * np.abs(want).max() and se.max() <= 1e-9 * np.abs(want).max()


def _align(x):
    return (x + 255) // 256 * 256


def test_restated_sizes_are_the_librarys():
    build.build(verbose=False)
    lib = _lib.load()
    for r in (2, 3, 11, 12, 63, 64):
        d = r + r * (r - 1) // 2
        assert lib.iq_kshap_pair_features(r) == d == kernelshap.pair_features(r) == ref.feature_count(r)
        for m in (1, 255, 256, 257, 4099, 65537, 1 << 20):
            for g in (1, 3, 10):
                want = _align(8 * d * d) + _align(8 * g * kernelshap.chunks(m)[0] * d) + _align(8 * (g + 1) * d) + 256
                assert lib.iq_kshap_pair_fit_scratch_bytes(m, r, g) == want == kernelshap.fit_scratch_bytes(m, r, g), (m, r, g)
    assert lib.iq_kshap_pair_features(1) == 0 and lib.iq_kshap_pair_features(65) == 0
    sb = lib.iq_kshap_pair_fit_scratch_bytes
    assert sb(0, 8, 1) == 0 and sb(10, 1, 1) == 0 and sb(10, 65, 1) == 0 and sb(10, 8, 0) == 0
    # the folds: units [0, U/2) and [U/2, U), whole units, at least two each
    assert kernelshap.fold_units(8, True) == (2, 2) and kernelshap.fold_units(10, True) == (2, 3) and kernelshap.fold_units(5, False) == (2, 3)
    for rows, paired in ((6, True), (3, False), (7, True)):
        with pytest.raises(_lib.IqError):
            kernelshap.fold_units(rows, paired)
    for rows, paired in ((600, True), (601, False), (10, True)):
        (a, b), (c, e) = ref.fold_rows(rows, paired)
        u0, u1 = kernelshap.fold_units(rows, paired)
        per = 2 if paired else 1
        assert (a, b, c, e) == (0, per * u0, per * u0, per * (u0 + u1)) and e == rows


def test_entry_points_are_declared_bound_and_exported_at_abi_122():
    build.build(verbose=False)
    lib = _lib.load()
    header = open(os.path.join(REPO, "include", "iq.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NAMES:
        assert name in _lib.SIGNATURES, name
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert hasattr(lib, name), name
    version = int(re.search(r"#define IQ_ABI_VERSION (\d+)", header).group(1))
    assert _lib.ABI_VERSION == lib.iq_version() == version >= 122
    assert " * 122:" in header and "Control variates for the all-pairs map" in header
    assert "iq_kshap_paircv.hip" in [os.path.basename(p) for p in build.sources()]
    # argument checks that need no device
    for m, r, g in ((0, 8, 1), (10, 1, 1), (10, 1025, 1), (10, 8, 0)):
        assert lib.iq_kshap_pairs_terms(None, None, None, None, m, r, g, None, None, 0, None) == -1, (m, r, g)
        assert b"iq_kshap_pairs_terms" in lib.iq_last_error()
        assert lib.iq_kshap_pair_shift_terms(None, None, None, None, m, r, g, None, None) == -1, (m, r, g)
    assert lib.iq_kshap_pairs_terms_se(None, None, None, 2, 8, 1, 1, None, None, None, 0, None) == -1           # one unit
    assert b"units" in lib.iq_last_error()
    assert lib.iq_kshap_pair_gram(None, 10, 65, None, None) == -1 and b"R=65" in lib.iq_last_error()
    assert lib.iq_kshap_pair_gram(None, 10, 8, None, None) == -1 and b"null pointer" in lib.iq_last_error()
    assert lib.iq_kshap_pair_fit(None, None, None, None, None, 1.0, 10, 65, 1, None, None, None, None, 0, None) == -1
    for ridge in (-1.0, float("nan")):
        assert lib.iq_kshap_pair_fit(None, None, None, None, None, ridge, 10, 8, 1, None, None, None, None, 0, None) == -1
        assert b"ridge" in lib.iq_last_error()
    assert lib.iq_kshap_pair_surrogate(None, None, None, None, 10, 65, 1, None, None, None) == -1


def test_both_parsers_take_control_and_leave_no_trace_without_it():
    from interpret_quality_amd import kernel_stage, wide_kernel_stage
    narrow = ["--model", "pointnet", "--num_regions", "8", "--samples", "40", "--pairs"]
    wide = ["--model", "pointnet", "--num_regions", "65", "--samples", "40", "--pairs"]
    for stage, argv, choices in ((kernel_stage, narrow, ("none", "shift", "regression")), (wide_kernel_stage, wide, ("none", "shift"))):
        without = vars(stage.make_args(argv))
        assert "control" not in without and kernel_stage.control_of(stage.make_args(argv)) == "none"
        for c in choices:
            with_flag = vars(stage.make_args(argv + ["--control", c]))
            assert with_flag["control"] == c and {k: v for k, v in with_flag.items() if k != "control"} == without
    for stage, argv in ((wide_kernel_stage, wide + ["--control", "regression"]),                  # no surrogate above 64 regions
                        (kernel_stage, narrow[:-1] + ["--control", "shift"]),                      # needs --pairs
                        (wide_kernel_stage, wide[:-1] + ["--control", "shift"]),
                        (kernel_stage, narrow[:4] + ["--samples", "all", "--pairs", "--control", "regression"]),
                        (kernel_stage, narrow + ["--control", "ridge"])):
        with pytest.raises(SystemExit):
            stage.make_args(argv)
    assert kernel_stage.make_args(narrow + ["--control", "none"]).control == "none"              # none needs nothing


def test_wrappers_refuse_before_they_touch_a_device():
    import argparse

    import torch
    from interpret_quality_amd import hip_ops
    assert wide_kernelshap.pairs_cv is kernelshap.pairs_cv
    assert kernelshap.CONTROLS == ("none", "shift", "regression") and wide_kernelshap.CONTROLS == ("none", "shift")
    keep = torch.zeros((8,), dtype=torch.int64)
    v, z = torch.zeros((1, 8)), torch.zeros((1,), dtype=torch.float64)
    with pytest.raises(_lib.IqError, match="shift"):
        hip_ops.kshap_pair_features(65)
    with pytest.raises(_lib.IqError, match="shift"):
        kernelshap.pairs_cv(torch.zeros((8, 2), dtype=torch.int64), v, 0.0, 1.0, 65, control="regression")
    with pytest.raises(_lib.IqError, match="weighted"):
        kernelshap.pairs_cv(keep, v, 0.0, 1.0, 8, weights=torch.ones(8, dtype=torch.float64))
    with pytest.raises(_lib.IqError, match="weighted"):
        hip_ops.kshap_pairs_terms_se(keep, torch.zeros((1, 8), dtype=torch.float64), 8, True, torch.ones(8, dtype=torch.float64))
    with pytest.raises(_lib.IqError, match="control"):
        kernelshap.pairs_cv(keep, v, 0.0, 1.0, 8, control="ridge")
    with pytest.raises(_lib.IqError, match="ridge"):
        kernelshap.pairs_cv(keep, v, 0.0, 1.0, 8, ridge=-1.0)
    with pytest.raises(_lib.IqError, match="4 units"):
        kernelshap.pairs_cv(keep[:6].contiguous(), v[:, :6].contiguous(), 0.0, 1.0, 8, paired=True)
    with pytest.raises(_lib.IqError):
        hip_ops.kshap_pair_gram(keep, 8)                                                          # CPU tensors
    with pytest.raises(_lib.IqError, match="narrow"):
        hip_ops.kshap_pair_gram(torch.zeros((8, 1), dtype=torch.int64), 8)
    args = argparse.Namespace(num_regions=8)
    with pytest.raises(_lib.IqError, match="pairs=True"):
        kernelshap.game(None, None, None, None, args, samples=40, control="shift")
    with pytest.raises(_lib.IqError, match="enumerated"):
        kernelshap.game(None, None, None, None, args, samples="all", pairs=True, control="shift")
    with pytest.raises(_lib.IqError, match="control"):
        wide_kernelshap.game(None, None, None, None, argparse.Namespace(num_regions=65), samples=40, pairs=True, control="regression")


def test_every_wrapper_that_lends_zeroed_memory_has_a_row_in_the_hostile_memory_table():
    """tests/test_guarded_alloc_cpu.py holds every hip_ops wrapper that allocates with ``torch.empty`` to a row of
    tests/test_workspace_contents_gpu.py.  The wrappers of this feature allocate their float64 scratch and outputs with
    ``torch.zeros`` instead and call ``torch.empty`` nowhere (a wrapper that does both is the other table's); this is the same
    completeness check for them, against the table of
    tests/test_kshap_paircv_gpu.py::test_results_do_not_depend_on_what_the_lent_memory_held."""
    import inspect

    from interpret_quality_amd import hip_ops
    import test_kshap_paircv_gpu as gpu_tests          # importing it touches no GPU
    lends = {n for n, f in vars(hip_ops).items() if inspect.isfunction(f) and f.__module__ == hip_ops.__name__
             and re.search(r"torch\.zeros\([^\n]*float64", inspect.getsource(f)) and "torch.empty(" not in inspect.getsource(f)}
    assert {"kshap_pair_gram", "kshap_pair_fit", "kshap_pairs_terms"} <= lends            # the scan sees them
    covered = {kind for kind, _, _, _ in gpu_tests.LENT}
    assert all(hasattr(hip_ops, k) for k in covered)
    assert not lends - covered, sorted(lends - covered)
