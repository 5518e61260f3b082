"""CPU: the all-pairs interaction estimator (SHAP-IQ on the regression rows; include/iq.h) - the host's coefficient
table against exact rationals, the NumPy restatement (tests/kshap_pairs_ref.py) against the identities that define it, the
chunk rule of the pairwise product, and the plumbing: the two entry points declared, bound and exported at ABI 120, their
argument checks, both drivers' --pairs flag."""
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import kshap_pairs_ref as ref
import wide_kernelshap_ref as wide_ref
from interpret_quality_amd import _lib, build, kernelshap, wide_kernelshap

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("iq_kshap_pairs_scratch_bytes", "iq_kshap_pairs")


@pytest.mark.parametrize("n", [2, 3, 4, 24, 64, 65, 1024])
def test_pair_coefficients_against_the_rational_table(n):
    got = kernelshap.pair_coefficients(n)
    want = ref.coefficients(n)
    assert got.shape == (n + 1, 3) and got.dtype == np.float64
    assert not got[0].any() and not got[n].any()
    assert got[1, 2] == 0.0 and got[n - 1, 0] == 0.0
    worst = 0.0
    for s in range(n + 1):
        for k in range(3):
            exact = want[s, k]
            if exact == 0:
                assert got[s, k] == 0.0, (s, k)
                continue
            err = abs(Fraction(got[s, k]) - exact) / Fraction(math.ulp(float(exact)))
            worst = max(worst, float(err))
    print("n=%d: worst entry %.2f ulp" % (n, worst))
    assert worst <= 4.0
    # the three coefficients give mu back: the table IS the estimator's weight
    m = ref.mu(n)
    for s in range(1, n):
        a, b, c = want[s]
        assert a + b == m[s, 1]
        if s <= n - 2:
            assert a == m[s, 0]
        if s >= 2:
            assert a + 2 * b + c == m[s, 2]


@pytest.mark.parametrize("n", [2, 3, 4, 7, 9])
def test_closed_form_of_mu_is_gamma_over_the_sampling_probability(n):
    a, b = ref.mu(n), ref.mu_from_gamma(n)
    for s in range(n + 1):
        for k in range(3):
            assert a[s, k] == b[s, k], (s, k)


def _integer_table(n, seed):
    """A float32 table of small integers: every float32 difference and every widening is exact."""
    return np.random.default_rng(seed).integers(-40, 41, size=1 << n).astype(np.float32)


@pytest.mark.parametrize("n", range(2, 11))
def test_enumerated_rows_give_the_exact_index_both_ways(n):
    """Enumerated rows with enumeration_weights: the defining sum is the exact SII, the mean over the orders of
    exact_ref.interactions - and the weighted alpha/beta/gamma form is the same sum."""
    v = _integer_table(n, 120 + n)
    keep, w = wide_ref.enumerated(n)
    rows = v[keep[:, 0].astype(np.int64)]
    delta = float(v[-1]) - float(v[0])
    direct = ref.pairs(keep, rows, v[0], delta, n, w)
    coef = ref.pairs_by_coefficients(keep, rows, v[0], delta, n, w)
    want = ref.exact_sii(v, n)
    scale = float(np.abs(v).max())
    print("n=%d: direct %.3g, coefficients %.3g of max|v|" % (n, np.abs(direct - want).max() / scale, np.abs(coef - want).max() / scale))
    assert np.abs(direct - want).max() <= 1e-12 * scale
    assert np.abs(coef - want).max() <= 1e-12 * scale
    assert np.array_equal(direct, direct.T) and not np.diag(direct).any()


@pytest.mark.parametrize("r", [3, 17, 65])
def test_pair_sums_are_the_exact_sums_and_both_forms_agree_on_sampled_rows(r):
    rng = np.random.RandomState(r)
    keep = np.concatenate([ref.size_law_rows(r, 40, rng), ref.edge_rows(r)])
    m = len(keep)
    v = rng.standard_normal(m).astype(np.float32)
    z = ref.rows_of(keep, r)
    zf = z.astype(np.float64)
    x = rng.standard_normal(m) * np.exp(rng.uniform(-6, 6, size=m))
    got = ref.pair_sums(zf, zf, x.astype(ref.L)).astype(np.float64)
    want = wide_ref.exact_sums(z, x[:, None] * zf)                    # [j][i] = sum_m z_mi (x_m z_mj), exactly, rounded once
    assert np.all(np.abs(got - want.T) <= m * 2.0 ** -ref.BITS * np.abs(x).max() + np.spacing(np.abs(want.T)))   # what pair_sums cuts off
    for weights in (None, rng.uniform(0.5, 2.0, size=m)):
        a = ref.pairs(keep, v, 0.25, 1.5, r, weights)
        b = ref.pairs_by_coefficients(keep, v, 0.25, 1.5, r, weights)
        bound = ref.bound(keep, v, 0.25, r, weights)
        print("R=%d: |direct - coefficients| = %.3g, bound %.3g" % (r, np.abs(a - b).max(), bound))
        assert bound > 0 and np.abs(a - b).max() <= 1e-3 * bound      # both exact: they differ by their last roundings only


def test_rows_of_size_0_and_r_contribute_nothing_but_count():
    r = 9
    full, empty = wide_ref.full_row(r), np.zeros(1, dtype=np.uint64)
    keep = np.array([full, empty, full, empty], dtype=np.uint64).reshape(4, 1)
    out = ref.pairs(keep, np.array([3.0, -2.0, 7.0, 1.0], dtype=np.float32), 0.5, 4.0, r)
    want = np.full((r, r), 4.0 / (r - 1))
    np.fill_diagonal(want, 0.0)
    assert np.array_equal(out, want)


def test_entry_points_are_declared_bound_and_exported_at_abi_120():
    build.build(verbose=False)
    lib = _lib.load()
    header = open(os.path.join(REPO, "include", "iq.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NAMES:
        assert name in _lib.SIGNATURES, name
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert hasattr(lib, name), name
    version = int(re.search(r"#define IQ_ABI_VERSION (\d+)", header).group(1))
    assert _lib.ABI_VERSION == lib.iq_version() == version >= 120
    assert " * 120:" in header
    sb = lib.iq_kshap_pairs_scratch_bytes
    assert sb(0, 128, 1) == 0 and sb(10, 1, 1) == 0 and sb(10, 1025, 1) == 0 and sb(10, 128, 0) == 0
    assert sb(10, 2, 1) > 0 and sb(10, 64, 1) > 0
    big = sb(1025000, 1024, 1)
    assert 0 < big <= (64 << 20) + lib.iq_kshap_scratch_bytes_wide(1025000, 1024, 1)
    assert big < sb(1025000, 1024, 3)
    # argument checks that need no device
    for m, r, g in ((0, 128, 1), (10, 1, 1), (10, 1025, 1), (10, 128, 0), (10, 128, 65536)):
        assert lib.iq_kshap_pairs(None, None, None, None, None, None, m, r, g, None, None, 0, None) == -1, (m, r, g)
        assert b"iq_kshap_pairs" in lib.iq_last_error()
    assert lib.iq_kshap_pairs(None, None, None, None, None, None, 10, 128, 1, None, None, 0, None) == -1
    assert b"null pointer" in lib.iq_last_error()


def _align(x):
    return (x + 255) // 256 * 256


def _scratch_by_the_rule(m, r, g):
    """The library's scratch size rebuilt from the restated chunk rules: row sizes (uint16), the product's partials on the blocks
    of 64 x 64 on or above the diagonal, the moment's partials, and the folded L, A and W_sum."""
    count, _ = kernelshap.chunks(m)
    qcount, _ = kernelshap.pair_chunks(m, r)
    nb = (r + 63) // 64
    blocks = nb * (nb + 1) // 2
    return (_align(2 * m) + _align(8 * g * qcount * blocks * 4096) + _align(8 * g * count * r) + _align(8 * g * count) + _align(8 * count)
            + _align(8 * g * r) + _align(8 * g) + 256)


def test_chunk_rule_is_a_pure_function_of_rows_and_regions():
    build.build(verbose=False)
    lib = _lib.load()
    for r in (2, 64, 65, 512, 1000, 1024):
        for m in (1, 255, 256, 257, 4097, 65537, 129000, 1025000, 1 << 24, 1 << 30):
            count, per = kernelshap.pair_chunks(m, r)
            assert (count, per) == kernelshap.pair_chunks(m, r)
            base = kernelshap.chunks(m)
            assert 1 <= count <= base[0] <= 256
            assert count * per * 256 >= m > (count - 1) * per * 256                 # whole tiles, every row in one chunk, none empty
            assert count * r * r * 8 <= kernelshap.PAIR_PARTIAL_BYTES
            if base[0] * r * r * 8 <= kernelshap.PAIR_PARTIAL_BYTES:
                assert (count, per) == base
            for g in (1, 3):                                                          # the library cuts by the same rule
                assert lib.iq_kshap_pairs_scratch_bytes(m, r, g) == _scratch_by_the_rule(m, r, g), (m, r, g)
    assert kernelshap.pair_chunks(1025000, 1024)[0] == 8
    assert kernelshap.pair_chunks(129000, 128) == kernelshap.chunks(129000)


def test_both_parsers_accept_pairs_and_leave_no_trace_without_it():
    from interpret_quality_amd import kernel_stage, wide_kernel_stage
    for stage, argv in ((kernel_stage, ["--model", "pointnet", "--num_regions", "8", "--samples", "40"]),
                        (wide_kernel_stage, ["--model", "pointnet", "--num_regions", "65", "--samples", "40"])):
        without, with_flag = vars(stage.make_args(argv)), vars(stage.make_args(argv + ["--pairs"]))
        assert "pairs" not in without and with_flag["pairs"] is True
        assert {k: v for k, v in with_flag.items() if k != "pairs"} == without
        assert not kernel_stage.wants_pairs(stage.make_args(argv)) and kernel_stage.wants_pairs(stage.make_args(argv + ["--pairs"]))
    args = kernel_stage.make_args(["--model", "pointnet", "--num_regions", "8", "--samples", "all", "--compare_exact", "--pairs"])
    assert args.samples == "all" and args.compare_exact and args.pairs


def test_wrappers_refuse_cpu_tensors_and_bad_shapes():
    import torch
    from interpret_quality_amd import hip_ops
    assert wide_kernelshap.pairs is kernelshap.pairs
    v, z = torch.zeros((1, 4)), torch.zeros((1,), dtype=torch.float64)
    with pytest.raises(_lib.IqError):
        hip_ops.kshap_pairs(torch.zeros((4,), dtype=torch.int64), v, z, z, 8)               # CPU tensors
    with pytest.raises(_lib.IqError, match=r"\(M, 2\)"):
        hip_ops.kshap_pairs(torch.zeros((4,), dtype=torch.int64), v, z, z, 128)             # narrow rows of a wide game
    with pytest.raises(_lib.IqError, match=r"\(B, 2\)"):
        hip_ops.kshap_pairs(torch.zeros((4, 1), dtype=torch.int64), v, z, z, 128)
    for bad in (1, 1025):
        with pytest.raises(_lib.IqError):
            hip_ops.kshap_pairs(torch.zeros((4,), dtype=torch.int64), v, z, z, bad)
    with pytest.raises(_lib.IqError):
        kernelshap.pair_coefficients(1)
