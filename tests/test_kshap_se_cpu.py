"""CPU: the standard errors of the sampled estimates (include/iq.h, "Standard errors") - the variance estimate is
unbiased, by enumerating the law of a unit in rationals; the one-product form P + B k + G [k = 2] the library computes is the
square of the unit's term at every feasible (s, k); and the plumbing: the entry points declared, bound and exported at ABI 121,
their scratch sizes against a restatement of the carve, their refusals, and the drivers' --se rules."""
import os
import re
from fractions import Fraction
from itertools import product

import numpy as np
import pytest

import kshap_pairs_ref as pairs_ref
import kshap_se_ref as ref
from interpret_quality_amd import _lib, build, kernelshap, wide_kernelshap

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("iq_kshap_pairs_se_scratch_bytes", "iq_kshap_pairs_se", "iq_kshap_moment_se_scratch_bytes_wide", "iq_kshap_moment_se_wide",
         "iq_shapley_sq_accum_games")


def _table(r, seed):
    return np.random.default_rng(seed).integers(-40, 41, size=1 << r).astype(np.float32)


def _variance(ys, rows):
    """(U / (U - 1)) (S2 - S1^2 / U) / M^2 of the units' values ``ys``, in rationals."""
    u = len(ys)
    s1, s2 = sum(ys), sum(y * y for y in ys)
    return Fraction(u, u - 1) * (s2 - s1 * s1 / u) / (rows * rows)


def _expectations(law, term, units, rows_per_unit):
    """Over all ordered draws of ``units`` iid units: (E[est - const], Var[est], E[var]) of est = const + (1/M) sum_u y_u."""
    m = units * rows_per_unit
    ys = [(p, term(mask)) for p, mask in law]
    mean = sum(p * y for p, y in ys)
    var_y = sum(p * (y - mean) ** 2 for p, y in ys)
    e_var = Fraction(0)
    for draw in product(ys, repeat=units):
        weight = Fraction(1)
        for p, _ in draw:
            weight *= p
        e_var += weight * _variance([y for _, y in draw], m)
    return mean * units / m, var_y * units / (m * m), e_var


@pytest.mark.parametrize("paired", [False, True])
@pytest.mark.parametrize("r", [4, 5])
def test_variance_estimate_is_unbiased_by_enumeration(r, paired):
    """U = 2 units, every ordered pair of them under P(S): the estimator's mean is the exact value and E[var] its true variance,
    in rationals, for two pairs and two regions.  Reading the two rows of a paired unit as two independent draws is not."""
    table = _table(r, 700 + r)
    law = ref.unit_law(r)
    c = 2 if paired else 1
    sii = pairs_ref.exact_sii(table, r)
    delta = int(table[-1]) - int(table[0])
    for i, j in ((0, 1), (1, r - 1)):
        mean, true_var, e_var = _expectations(law, lambda mask: ref.pair_term(table, mask, i, j, r, paired), 2, c)
        assert abs(float(mean + Fraction(delta, r - 1)) - sii[i, j]) <= 1e-12 * np.abs(table).max()
        assert e_var == true_var and true_var > 0, (i, j)
        if paired:                       # the wrong reading: 2 U rows as 2 U units of their own
            def rows_as_units(draw):
                flat = [t for _, mask in draw for t in ref.pair_term(table, mask, i, j, r, True, independent=True)]
                return _variance(flat, len(flat))
            wrong = Fraction(0)
            for draw in product(law, repeat=2):
                wrong += draw[0][0] * draw[1][0] * rows_as_units(draw)
            assert wrong != true_var, (i, j)
    import exact_ref
    phi = exact_ref.shapley(table, r) if hasattr(exact_ref, "shapley") else None
    for i in (0, r - 1):
        mean, true_var, e_var = _expectations(law, lambda mask: ref.phi_term(table, mask, i, r, paired), 2, c)
        assert e_var == true_var and true_var > 0, i
        if phi is not None:
            assert abs(float(mean + Fraction(delta, r)) - phi[i]) <= 1e-12 * np.abs(table).max()


@pytest.mark.parametrize("paired", [False, True])
def test_the_restatement_on_rows_is_the_rational_variance(paired):
    """ref.pairs_var / ref.phi_var on concrete rows against the rational formula on the same units."""
    r = 5
    table = _table(r, 31)
    rng = np.random.RandomState(3)
    masks = [int(m) for m in rng.randint(1, (1 << r) - 1, size=6)]
    full = (1 << r) - 1
    keep = np.array([[m, full & ~m] if paired else [m] for m in masks], dtype=np.uint64).reshape(-1, 1)
    v = table[keep[:, 0].astype(np.int64)]
    rows = len(keep)
    got = ref.pairs_var(keep, v, table[0], r, paired)
    for i, j in ((0, 1), (2, 4)):
        want = _variance([ref.pair_term(table, m, i, j, r, paired) for m in masks], rows)
        assert abs(got[i, j] - float(want)) <= 1e-14 * float(want) and got[i, j] == got[j, i]
    assert not np.diag(got).any()
    got = ref.phi_var(keep, v, table[0], r, paired)
    for i in range(r):
        want = _variance([ref.phi_term(table, m, i, r, paired) for m in masks], rows)
        assert abs(got[i] - float(want)) <= 1e-14 * float(want)


@pytest.mark.parametrize("r", [2, 3, 4, 9, 64, 65])
def test_one_product_form_is_the_square_at_every_feasible_case(r):
    """x(k)^2 = P + B k + G [k = 2] with P = x(0)^2, B = x(1)^2 - x(0)^2, G = x(2)^2 - 2 x(1)^2 + x(0)^2, for the mu of every size
    with the impossible cases set to 0 (k = 2 at s = 1, k = 0 at s = R - 1), paired and unpaired, in rationals."""
    mu = pairs_ref.mu(r)
    d0, d1 = Fraction(7, 3), Fraction(-5, 11)
    for s in range(1, r):
        for paired in (False, True):
            x = [d0 * mu[s, k] + (d1 * mu[r - s, 2 - k] if paired else 0) for k in range(3)]
            p, b, g = x[0] ** 2, x[1] ** 2 - x[0] ** 2, x[2] ** 2 - 2 * x[1] ** 2 + x[0] ** 2
            for k in range(3):
                if k <= s and 2 - k <= r - s:                        # a row of s regions can hold k of a pair's two
                    assert p + b * k + g * (k == 2) == x[k] ** 2, (s, k, paired)
            if s == 1:
                assert mu[s, 2] == 0
            if s == r - 1:
                assert mu[s, 0] == 0


def test_entry_points_are_declared_bound_and_exported_at_abi_121():
    build.build(verbose=False)
    lib = _lib.load()
    header = open(os.path.join(REPO, "include", "iq.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NAMES:
        assert name in _lib.SIGNATURES, name
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert hasattr(lib, name), name
    version = int(re.search(r"#define IQ_ABI_VERSION (\d+)", header).group(1))
    assert _lib.ABI_VERSION == lib.iq_version() == version >= 121
    assert " * 121:" in header
    from interpret_quality_amd import classwise, hip_ops
    for fn in ("kshap_pairs_se", "kshap_moment_se", "shapley_sq_accum_games"):
        assert callable(getattr(hip_ops, fn))
    assert wide_kernelshap.pairs_se is kernelshap.pairs_se and callable(kernelshap.phi_se) and callable(wide_kernelshap.phi_se)
    assert "se" in classwise.shapley.__code__.co_varnames
    # refusals that need no device: one unit, odd rows in pairs, arguments out of range
    for sb in (lib.iq_kshap_pairs_se_scratch_bytes, lib.iq_kshap_moment_se_scratch_bytes_wide):
        assert sb(1, 8, 1, 0) == 0 and sb(2, 8, 1, 1) == 0 and sb(5, 8, 1, 1) == 0 and sb(4, 1, 1, 0) == 0 and sb(4, 1025, 1, 0) == 0 and sb(4, 8, 0, 0) == 0
        assert sb(2, 8, 1, 0) > 0 and sb(4, 8, 1, 1) > 0
    for m, paired in ((1, 0), (2, 1), (5, 1)):
        assert lib.iq_kshap_pairs_se(None, None, None, None, None, m, 8, 1, paired, None, None, None, 0, None) == -1
        assert b"iq_kshap_pairs_se" in lib.iq_last_error() and b"units" in lib.iq_last_error()
        assert lib.iq_kshap_moment_se_wide(None, None, None, m, 8, 1, paired, None, None, None, 0, None) == -1
        assert b"iq_kshap_moment_se_wide" in lib.iq_last_error() and b"units" in lib.iq_last_error()
    assert lib.iq_kshap_pairs_se(None, None, None, None, None, 4, 8, 1, 1, None, None, None, 0, None) == -1
    assert b"null pointer" in lib.iq_last_error()
    assert lib.iq_shapley_sq_accum_games(None, 0, None, None, None, 0, None, 0, 1, 1, None, 0, None) == -1
    assert b"iq_shapley_sq_accum_games" in lib.iq_last_error()


def _align(x):
    return (x + 255) // 256 * 256


def _pairs_se_scratch(m, r, g, paired):
    """iq_kshap_pairs's scratch, then the units' (P, B, G), the second product's partials on pair_chunks(U, R), the second moment's
    and scalar's partials on chunks(U), their folds and the fold kernel's count."""
    u = m // 2 if paired else m
    count, _ = kernelshap.chunks(u)
    qcount, _ = kernelshap.pair_chunks(u, r)
    nb = (r + 63) // 64
    blocks = nb * (nb + 1) // 2
    return (_lib.load().iq_kshap_pairs_scratch_bytes(m, r, g) + _align(8 * 3 * g * u) + _align(8 * g * qcount * blocks * 4096)
            + _align(8 * g * count * r) + _align(8 * g * count) + _align(8 * g * r) + _align(8 * g) + 256)


def _moment_se_scratch(m, r, g, paired):
    """iq_kshap_moment_wide's scratch, then its wsum, the units' (e, f) and their partials on chunks(U)."""
    u = m // 2 if paired else m
    count, _ = kernelshap.chunks(u)
    return _lib.load().iq_kshap_scratch_bytes_wide(m, r, g) + 256 + _align(8 * 2 * g * u) + _align(8 * g * count * r) + _align(8 * g * count)


def test_scratch_sizes_follow_the_restated_carve():
    build.build(verbose=False)
    lib = _lib.load()
    for r in (2, 64, 65, 1000, 1024):
        for m in (2, 4, 256, 514, 4098, 131074, 1025000, 1 << 24):
            for g in (1, 3):
                for paired in (0, 1):
                    if m // (1 + paired) < 2:                                       # one unit: refused
                        assert lib.iq_kshap_pairs_se_scratch_bytes(m, r, g, paired) == 0 == lib.iq_kshap_moment_se_scratch_bytes_wide(m, r, g, paired)
                        continue
                    assert lib.iq_kshap_pairs_se_scratch_bytes(m, r, g, paired) == _pairs_se_scratch(m, r, g, paired), (m, r, g, paired)
                    assert lib.iq_kshap_moment_se_scratch_bytes_wide(m, r, g, paired) == _moment_se_scratch(m, r, g, paired), (m, r, g, paired)
    assert lib.iq_kshap_pairs_se_scratch_bytes(2, 8, 1, 1) == 0


def _refused(stage, argv):
    with pytest.raises(SystemExit):
        stage.make_args(argv)


def test_parsers_take_se_and_leave_no_trace_without_it(capsys):
    from interpret_quality_amd import class_stage, kernel_stage, wide_kernel_stage
    narrow = ["--model", "pointnet", "--num_regions", "8", "--samples", "40"]
    wide = ["--model", "pointnet", "--num_regions", "65", "--samples", "40"]
    for stage, argv in ((kernel_stage, narrow + ["--gram", "analytic"]), (kernel_stage, narrow + ["--pairs"]), (wide_kernel_stage, wide),
                        (class_stage, ["--model", "pointnet", "--num_regions", "8"]),
                        (class_stage, ["--model", "pointnet", "--num_regions", "65", "--estimator", "kernel"])):
        without, with_flag = vars(stage.make_args(argv)), vars(stage.make_args(argv + ["--se"]))
        assert "se" not in without and with_flag["se"] is True
        assert {k: v for k, v in with_flag.items() if k != "se"} == without
        assert kernel_stage.wants_se(stage.make_args(argv + ["--se"])) and not kernel_stage.wants_se(stage.make_args(argv))
    _refused(kernel_stage, narrow + ["--se"])                                        # the sampled Gram matrix and no --pairs
    assert "sampled" in capsys.readouterr().err
    _refused(kernel_stage, ["--model", "pointnet", "--num_regions", "8", "--samples", "all", "--gram", "analytic", "--se"])
    assert "--samples all" in capsys.readouterr().err
    _refused(kernel_stage, ["--model", "pointnet", "--num_regions", "8", "--samples", "all", "--pairs", "--se"])
    _refused(class_stage, ["--model", "pointnet", "--num_regions", "8", "--estimator", "kernel", "--se"])
    _refused(class_stage, ["--model", "pointnet", "--num_regions", "8", "--num_samples", "1", "--se"])
    capsys.readouterr()


def test_wrappers_refuse_before_any_launch():
    import argparse
    import torch
    from interpret_quality_amd import hip_ops
    z = torch.zeros((1,), dtype=torch.float64)
    keep, v = torch.zeros((4,), dtype=torch.int64), torch.zeros((1, 4))
    with pytest.raises(_lib.IqError):
        hip_ops.kshap_pairs_se(keep, v, z, z, 8)                                     # CPU tensors
    with pytest.raises(_lib.IqError, match=r"\(M, 2\)"):
        hip_ops.kshap_pairs_se(keep, v, z, z, 128)                                   # narrow rows of a wide game
    with pytest.raises(_lib.IqError, match="weighted"):
        hip_ops.kshap_pairs_se(keep, v, z, z, 8, True, torch.ones(4, dtype=torch.float64))
    with pytest.raises(_lib.IqError, match="weighted"):
        hip_ops.kshap_moment_se(keep, v, z, 8, True, torch.ones(4, dtype=torch.float64))
    args = argparse.Namespace(num_regions=8)
    with pytest.raises(_lib.IqError, match="enumerated"):
        kernelshap.game(None, None, None, None, args, samples="all", gram="analytic", se=True)
    with pytest.raises(_lib.IqError, match="analytic"):
        kernelshap.game(None, None, None, None, args, samples=40, gram="sampled", se=True)
    with pytest.raises(_lib.IqError, match="enumerated"):
        wide_kernelshap.game(None, None, None, None, argparse.Namespace(num_regions=65), samples="all", se=True)
    with pytest.raises(_lib.IqError, match="2 permutations"):
        hip_ops.shapley_se(np.zeros(3), np.zeros(3), 1)
    assert np.array_equal(hip_ops.shapley_se(np.array([2.0, 4.0]), np.array([4.0, 10.0]), 2), ref.shapley_se(np.array([2.0, 4.0]), np.array([4.0, 10.0]), 2))
