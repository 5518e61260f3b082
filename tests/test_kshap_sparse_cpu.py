"""CPU: the sparse regression control variate (include/iq.h, "Sparse regression control variate") - the closed form
of the sparse game generator against the enumerated index, the identity that makes the control unbiased on the NumPy
restatement (tests/kshap_sparse_ref.py), ``neighbour_pairs``, the refusals that need no device, both drivers' flags and the
plumbing: the entry points declared, bound and exported at ABI 123, their argument checks, and that the new wrappers allocate
zeroed memory only."""
import argparse
import inspect
import os
import re

import numpy as np
import pytest
import torch

import kshap_paircv_ref as cv_ref
import kshap_pairs_ref as pairs_ref
import kshap_sparse_ref as ref
import wide_kernelshap_ref as wide_ref
from interpret_quality_amd import _lib, build, hip_ops, kernel_stage, kernelshap, sparse_ops, wide_kernel_stage, wide_kernelshap

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("iq_kshap_sparse_expand", "iq_kshap_feat_gram", "iq_kshap_feat_fit_scratch_bytes", "iq_kshap_feat_fit",
         "iq_kshap_feat_surrogate")


@pytest.mark.parametrize("n", range(3, 11))
def test_closed_form_of_the_generator_is_the_enumerated_index(n):
    """I_ij = sum_{T holding i, j} c_T / (|T| - 1) against kshap_pairs_ref.exact_sii of the game's own value table.  Integer
    coefficients: the table is exact in float32; the index is compared to 2^-40 of its scale (exact_sii averages in float64)."""
    game = ref.random_game(n, np.random.RandomState(900 + n))
    table = game.table()
    assert np.array_equal(table.astype(np.float32).astype(np.float64), table)
    assert table[0] == game.v_empty and table[-1] == game.v_full
    want = pairs_ref.exact_sii(table.astype(np.float32), n)
    got = game.index()
    assert np.array_equal(got, got.T) and not np.diag(got).any()
    assert np.abs(got - want).max() <= 2.0 ** -40 * max(1.0, np.abs(want).max()), n
    assert any(len(t) >= 3 for t in game.sets) and np.abs(got).max() > 0


def _sparse_list(n, rng):
    full = ref.complete_list(n)
    keep = np.sort(rng.choice(len(full), size=len(full) // 2, replace=False))
    return full[keep]


@pytest.mark.parametrize("n", range(2, 9))
def test_any_sparse_surrogate_leaves_the_enumerated_estimate_exact(n):
    """Over the enumerated rows with enumeration weights the estimator is its expectation: C(beta) + (delta - sum beta) / (n-1) +
    SHAPIQ(v - v0 - g_beta) is the exact index for ANY beta on ANY list, to kshap_pairs_ref.bound on the residual terms."""
    rng = np.random.RandomState(n)
    v = np.random.default_rng(620 + n).integers(-40, 41, size=1 << n).astype(np.float32)
    keep, w = wide_ref.enumerated(n)
    rows = v[keep[:, 0].astype(np.int64)]
    delta = float(v[-1]) - float(v[0])
    want = pairs_ref.exact_sii(v, n)
    for pairs in (np.zeros((0, 2), dtype=np.int32), _sparse_list(n, rng), ref.complete_list(n)):
        d = n + len(pairs)
        for name, beta in (("zero", np.zeros(d)), ("random", rng.standard_normal(d) * 10.0), ("huge", rng.standard_normal(d) * 1e12)):
            got, t = ref.with_surrogate(keep, rows, v[0], delta, beta, n, pairs, w)
            tol = cv_ref.bound(keep, t, n, w)
            err = np.abs(got - want).max()
            print("n=%d K=%d %s: error %.3g, tolerance %.3g" % (n, len(pairs), name, err, tol))
            assert err <= tol, (n, len(pairs), name)
            assert np.array_equal(got, got.T) and not np.diag(got).any()


def test_restatement_with_the_complete_list_is_the_regression_restatement():
    """Features, Gram matrix, fit and estimate of the complete row-major list are those of tests/kshap_paircv_ref.py."""
    rng = np.random.RandomState(4)
    for r in (2, 3, 6):
        keep = pairs_ref.size_law_rows(r, 40, rng)
        full = ref.complete_list(r)
        f = ref.expand(keep, full, r)
        assert np.array_equal(f, cv_ref.features(keep, r)) and np.array_equal(ref.gram(f), cv_ref.gram(keep, r))
        assert np.array_equal(ref.pack(f)[:, 0] & np.uint64((1 << r) - 1), keep[:, 0])
        v = rng.standard_normal(len(keep)).astype(np.float32)
        assert np.array_equal(ref.fit(f, v, 0.25, 1.5, 0.5), cv_ref.fit(keep[:, 0], v, 0.25, 1.5, r, 0.5))
        beta = rng.standard_normal(f.shape[1])
        assert np.array_equal(ref.pair_map(beta, r, full), cv_ref.pair_map(beta, r))
        assert np.array_equal(kernelshap.sparse_coefficient_map(beta, r, full), cv_ref.pair_map(beta, r))
        out, se, _ = ref.pairs_cv(keep, v, 0.25, 1.5, r, full)
        want, want_se = cv_ref.pairs_cv(keep, v, 0.25, 1.5, r)
        assert np.array_equal(out, want) and np.array_equal(se, want_se)


def test_restatement_returns_a_listed_game_exactly():
    """Singles and LISTED pairs with integer coefficients, ridge 0: every fold's fit is the game, the residuals vanish."""
    r, rng = 9, np.random.RandomState(12)
    pairs = _sparse_list(r, rng)
    game = ref.SparseGame(r, [(i,) for i in range(r)] + [tuple(p) for p in pairs], rng.randint(-5, 6, size=r + len(pairs)), base=2.0)
    keep = pairs_ref.size_law_rows(r, 200, rng)
    v = game.values(keep).astype(np.float32)
    out, se, beta = ref.pairs_cv(keep, v, game.v_empty, game.v_full - game.v_empty, r, pairs, ridge=0.0)
    top = np.abs(game.index()).max()
    assert np.abs(out - game.index()).max() <= 1e-9 * top and se.max() <= 1e-9 * top
    assert np.abs(beta - game.coef[None]).max() <= 1e-9 * np.abs(game.coef).max()


def test_neighbour_pairs():
    rng = np.random.RandomState(2)
    c = rng.standard_normal((9, 3))
    for k in (0, 1, 7, 36):
        got = kernelshap.neighbour_pairs(c, k)
        assert got.shape == (k, 2) and got.dtype == np.int32 and np.array_equal(got, ref.neighbour_pairs(c, k))
        sparse_ops.check_pair_list(got, 9)                           # sorted row-major, i < j: a pair list as it stands
    assert np.array_equal(kernelshap.neighbour_pairs(c, 36), ref.complete_list(9))
    assert np.array_equal(kernelshap.neighbour_pairs(torch.from_numpy(c), 7), kernelshap.neighbour_pairs(c, 7))
    # ties: the corners of a square - four sides of length 1, two diagonals; among equals the lexicographically smaller pair
    square = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], dtype=np.float32)
    assert kernelshap.neighbour_pairs(square, 1).tolist() == [[0, 1]]
    assert kernelshap.neighbour_pairs(square, 2).tolist() == [[0, 1], [0, 3]]
    assert kernelshap.neighbour_pairs(square, 3).tolist() == [[0, 1], [0, 3], [1, 2]]
    assert kernelshap.neighbour_pairs(square, 4).tolist() == [[0, 1], [0, 3], [1, 2], [2, 3]]
    assert kernelshap.neighbour_pairs(square, 5).tolist() == [[0, 1], [0, 2], [0, 3], [1, 2], [2, 3]]
    assert kernelshap.neighbour_pairs(np.zeros((5, 3)), 3).tolist() == [[0, 1], [0, 2], [0, 3]]          # all equal: the first three
    # float64 on the host: a difference float32 cannot see decides
    close = np.array([[0, 0, 0], [1.0, 0, 0], [0, 1.0 + 1e-12, 0]], dtype=np.float64)
    assert kernelshap.neighbour_pairs(close, 1).tolist() == [[0, 1]]
    assert kernelshap.neighbour_pairs(close[[0, 2, 1]], 1).tolist() == [[0, 2]]
    for bad_k in (-1, 37):
        with pytest.raises(_lib.IqError):
            kernelshap.neighbour_pairs(c, bad_k)
    assert kernelshap.default_control_pairs(130) == 390 and kernelshap.default_control_pairs(1024) == 1056
    assert kernelshap.default_control_pairs(8) == 24 and kernelshap.default_control_pairs(3) == 3


def test_refusals_that_need_no_device():
    assert wide_kernelshap.pairs_cv is kernelshap.pairs_cv
    assert kernelshap.CONTROLS == ("none", "shift", "regression") and wide_kernelshap.CONTROLS == ("none", "shift")
    assert kernelshap.LIST_CONTROLS == wide_kernelshap.LIST_CONTROLS == ("sparse",)
    keep = torch.zeros((8,), dtype=torch.int64)
    v = torch.zeros((1, 8))
    for what, pairs in (("increasing", [[0, 2], [0, 1]]),                 # unsorted
                        ("increasing", [[0, 1], [0, 1]]),                 # a duplicated pair
                        ("i < j", [[1, 1]]), ("i < j", [[2, 1]]),         # i >= j
                        ("i < j", [[0, 8]]), ("i < j", [[-1, 3]]),        # out of range
                        ("K,2", [[0, 1, 2]]), ("K,2", [[0.0, 1.0]])):
        with pytest.raises(_lib.IqError, match=what):
            kernelshap.pairs_cv(keep, v, 0.0, 1.0, 8, control="sparse", pair_list=pairs)
        with pytest.raises(_lib.IqError, match=what):
            sparse_ops.kshap_sparse_expand(keep, pairs, 8)
    with pytest.raises(_lib.IqError, match="2080"):                       # d > 2080
        sparse_ops.check_pair_list(ref.complete_list(65)[:2016], 65)
    assert len(sparse_ops.check_pair_list(ref.complete_list(65)[:2015], 65)) == 2015
    with pytest.raises(_lib.IqError, match="2080"):
        kernelshap.pairs_cv(torch.zeros((8, 16), dtype=torch.int64), v, 0.0, 1.0, 1024, control="sparse",
                            pair_list=ref.complete_list(1024)[:1057])
    with pytest.raises(_lib.IqError, match="4 units"):                    # fewer than 4 units
        kernelshap.pairs_cv(keep[:6].contiguous(), v[:, :6].contiguous(), 0.0, 1.0, 8, control="sparse", pair_list=[[0, 1]])
    with pytest.raises(_lib.IqError, match="4 units"):
        kernelshap.pairs_cv(keep[:3].contiguous(), v[:, :3].contiguous(), 0.0, 1.0, 8, False, "sparse", pair_list=[])
    with pytest.raises(_lib.IqError, match="pair_list"):                  # the list and the control belong together
        kernelshap.pairs_cv(keep, v, 0.0, 1.0, 8, control="sparse")
    with pytest.raises(_lib.IqError, match="pair_list"):
        kernelshap.pairs_cv(keep, v, 0.0, 1.0, 8, control="regression", pair_list=[[0, 1]])
    with pytest.raises(_lib.IqError, match="ridge"):
        kernelshap.pairs_cv(keep, v, 0.0, 1.0, 8, control="sparse", ridge=-1.0, pair_list=[[0, 1]])
    with pytest.raises(_lib.IqError, match="weighted"):
        kernelshap.pairs_cv(keep, v, 0.0, 1.0, 8, control="sparse", pair_list=[], weights=torch.ones(8, dtype=torch.float64))
    with pytest.raises(_lib.IqError, match="CUDA"):                       # CPU tensors, after the list is accepted
        sparse_ops.kshap_sparse_expand(keep, [[0, 1]], 8)
    with pytest.raises(_lib.IqError, match="feat must be"):
        sparse_ops.kshap_feat_gram(torch.zeros((8, 2), dtype=torch.int64), 9)
    with pytest.raises(_lib.IqError, match="features"):
        sparse_ops.kshap_feat_gram(torch.zeros((8, 33), dtype=torch.int64), 2081)
    # the regression control above 64 regions still names the shift, and now the sparse control too
    with pytest.raises(_lib.IqError, match="shift") as e:
        hip_ops.kshap_pair_features(65)
    assert "sparse" in str(e.value)
    # game / play: refused before anything is drawn
    args = argparse.Namespace(num_regions=8)
    with pytest.raises(_lib.IqError, match="pairs=True"):
        kernelshap.game(None, None, None, None, args, samples=40, control="sparse")
    with pytest.raises(_lib.IqError, match="control_pairs"):
        kernelshap.game(None, None, None, None, args, samples=40, pairs=True, control="shift", control_pairs=3)
    with pytest.raises(_lib.IqError, match="centres"):
        kernelshap.game(None, None, None, None, args, samples=40, pairs=True, control="sparse", control_pairs=3)
    with pytest.raises(_lib.IqError, match="control_pairs=29"):
        kernelshap.game(None, None, None, None, args, samples=40, pairs=True, control="sparse", control_pairs=29, centres=np.zeros((8, 3)))
    with pytest.raises(_lib.IqError, match="increasing"):
        kernelshap.game(None, None, None, None, args, samples=40, pairs=True, control="sparse", control_pairs=[[0, 2], [0, 1]])
    with pytest.raises(_lib.IqError, match="increasing"):
        wide_kernelshap.game(None, None, None, None, argparse.Namespace(num_regions=65), samples=40, pairs=True, control="sparse",
                             control_pairs=[[0, 2], [0, 1]])


def test_both_parsers_take_the_sparse_control_and_leave_no_trace_without_it():
    narrow = ["--model", "pointnet", "--num_regions", "8", "--samples", "40", "--pairs"]
    wide = ["--model", "pointnet", "--num_regions", "65", "--samples", "40", "--pairs"]
    for stage, argv, n in ((kernel_stage, narrow, 8), (wide_kernel_stage, wide, 65)):
        without = vars(stage.make_args(argv))
        assert "control" not in without and "control_pairs" not in without
        assert kernel_stage.control_pairs_of(stage.make_args(argv)) is None
        only = stage.make_args(argv + ["--control", "sparse"])
        assert only.control == "sparse" and "control_pairs" not in vars(only)
        assert {k: v for k, v in vars(only).items() if k != "control"} == without
        assert kernel_stage.control_pairs_of(only) == kernelshap.default_control_pairs(n) == min(3 * n, 2080 - n, n * (n - 1) // 2)
        both = stage.make_args(argv + ["--control", "sparse", "--control_pairs", "5"])
        assert both.control_pairs == 5 and kernel_stage.control_pairs_of(both) == 5
        assert {k: v for k, v in vars(both).items() if k not in ("control", "control_pairs")} == without
        assert stage.make_args(argv + ["--control", "sparse", "--control_pairs", "0"]).control_pairs == 0
        for extra in (["--control_pairs", "5"],                                          # without --control sparse
                      ["--control", "shift", "--control_pairs", "5"],
                      ["--control", "sparse", "--control_pairs", "-1"],                  # K < 0
                      ["--control", "sparse", "--control_pairs", str(2081 - n)],         # R + K > 2080
                      ["--control", "sparse", "--control_pairs", "x"]):
            with pytest.raises(SystemExit):
                stage.make_args(argv + extra)
        with pytest.raises(SystemExit):
            stage.make_args(argv[:-1] + ["--control", "sparse"])                         # needs --pairs
    assert wide_kernel_stage.make_args(wide + ["--control", "sparse", "--control_pairs", "2015"]).control_pairs == 2015
    with pytest.raises(SystemExit):
        wide_kernel_stage.make_args(wide + ["--control", "regression"])                  # stays a parser error on the wide driver
    with pytest.raises(SystemExit):
        kernel_stage.make_args(narrow[:4] + ["--samples", "all", "--pairs", "--control", "sparse"])
    top = ["--model", "pointnet", "--num_regions", "1024", "--samples", "40", "--pairs", "--control", "sparse"]
    assert kernel_stage.control_pairs_of(wide_kernel_stage.make_args(top)) == 1056


def test_entry_points_are_declared_bound_and_exported_at_abi_123():
    build.build(verbose=False)
    lib = _lib.load()
    header = open(os.path.join(REPO, "include", "iq.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NAMES:
        assert name in _lib.SIGNATURES, name
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert hasattr(lib, name), name
    version = int(re.search(r"#define IQ_ABI_VERSION (\d+)", header).group(1))
    assert _lib.ABI_VERSION == lib.iq_version() == version >= 123
    assert " * 123:" in header and "Sparse regression control variate" in header
    assert int(re.search(r"#define IQ_KSHAP_SPARSE_MAX_FEATURES (\d+)", header).group(1)) == 2080 == sparse_ops.MAX_FEATURES
    assert "does not depend on the rewards" in re.sub(r"\s+\*?\s*", " ", header).lower()          # the unbiasedness condition
    names = [os.path.basename(p) for p in build.sources()]
    assert "iq_kshap_sparsecv.hip" in names and "iq_kshap_paircv.hip" in names
    # the fit's kernels exist once: the sparse file launches none of its own
    sparse_src = open(os.path.join(REPO, "interpret_quality_amd", "csrc", "iq_kshap_sparsecv.hip")).read()
    assert "fit_from_partials" in sparse_src and "#pragma clang fp contract(off)" in sparse_src
    for kernel in ("potrf", "trsm", "syrk", "solve_kernel", "constrain_kernel", "ridge_kernel"):
        assert kernel not in sparse_src, kernel
    # argument checks that need no device: -1 with null pointers
    for m, r, k in ((0, 8, 1), (10, 1, 0), (10, 1025, 0), (10, 8, -1), (10, 8, 2073), (10, 1024, 1057)):
        assert lib.iq_kshap_sparse_expand(None, None, m, r, k, None, None) == -1, (m, r, k)
        assert b"iq_kshap_sparse_expand" in lib.iq_last_error()
    assert lib.iq_kshap_sparse_expand(None, None, 10, 8, 0, None, None) == -1 and b"null pointer" in lib.iq_last_error()
    for m, d, g in ((0, 8, 1), (10, 1, 1), (10, 2081, 1), (10, 8, 0), (10, 8, 65536)):
        assert lib.iq_kshap_feat_gram(None, m, d, None, None) == -1, (m, d)
        assert lib.iq_kshap_feat_fit(None, None, None, None, None, 1.0, m, d, g, None, None, None, None, 0, None) == -1, (m, d, g)
        assert b"iq_kshap_feat_fit" in lib.iq_last_error()
        assert lib.iq_kshap_feat_surrogate(None, None, None, None, m, d, g, None, None, None) == -1, (m, d, g)
        assert lib.iq_kshap_feat_fit_scratch_bytes(m, d, g) == 0
    assert lib.iq_kshap_feat_gram(None, 10, 8, None, None) == -1 and b"null pointer" in lib.iq_last_error()
    assert lib.iq_kshap_feat_fit(None, None, None, None, None, 1.0, 10, 8, 1, None, None, None, None, 0, None) == -1
    assert b"null pointer" in lib.iq_last_error()
    for ridge in (-1.0, float("nan")):
        assert lib.iq_kshap_feat_fit(None, None, None, None, None, ridge, 10, 8, 1, None, None, None, None, 0, None) == -1
        assert b"ridge" in lib.iq_last_error()
    assert lib.iq_kshap_feat_surrogate(None, None, None, None, 10, 8, 1, None, None, None) == -1 and b"null pointer" in lib.iq_last_error()
    # the scratch is that of the regression fit with the same d
    for r in (2, 12, 64):
        d = r + r * (r - 1) // 2
        for m in (1, 257, 65537):
            for g in (1, 3):
                assert lib.iq_kshap_feat_fit_scratch_bytes(m, d, g) == lib.iq_kshap_pair_fit_scratch_bytes(m, r, g) > 0
    assert lib.iq_kshap_feat_fit_scratch_bytes(1 << 20, 2080, 10) == kernelshap.fit_scratch_bytes(1 << 20, 64, 10)


def test_the_new_wrappers_lend_zeroed_memory_only():
    src = inspect.getsource(sparse_ops)
    assert "torch.empty(" not in src and "empty_like" not in src and "new_empty" not in src
    lends = {n for n, f in vars(sparse_ops).items() if inspect.isfunction(f) and f.__module__ == sparse_ops.__name__
             and re.search(r"torch\.zeros\(", inspect.getsource(f))}
    assert lends == {"kshap_sparse_expand", "kshap_feat_gram", "kshap_feat_fit", "kshap_feat_surrogate"}
    import test_kshap_sparse_gpu as gpu_tests          # importing it touches no GPU
    assert {kind for kind, _, _ in gpu_tests.LENT} == lends          # each has its rows in the hostile-memory table
    # and hip_ops gained no allocating function: its control-variate wrappers are the ones it had
    assert not [n for n in vars(hip_ops) if "sparse" in n or "feat_" in n]
