"""CPU: the regression (KernelSHAP) estimator - the NumPy restatement of its contract (tests/kernelshap_ref.py) against the
identities that define it, the host-side pieces of interpret_quality_amd/kernelshap.py against the restatement, and the
plumbing: entry points declared, bound and exported, the driver's parser."""
import os
import re

import numpy as np
import pytest

import exact_ref
import kernelshap_ref as ref
from interpret_quality_amd import _lib, build

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("iq_kshap_keep_masks", "iq_kshap_accum", "iq_kshap_solve", "iq_kshap_scratch_bytes")


def _grid_table(n, seed):
    """A random float32 table on the grid 2^-10: every difference of two entries is a multiple of 2^-10 below 2^5, exact in float32,
    so the float32 marginals exact_ref.shapley takes (as the kernels and the reference do) are the table's exact marginals."""
    return (np.round(np.random.default_rng(seed).standard_normal(1 << n) * 1024) / 1024).astype(np.float32)


@pytest.mark.parametrize("n", range(2, 9))
def test_enumerated_weights_give_the_exact_shapley_vector(n):
    """The enumeration identity: all 2^n - 2 proper coalitions with w(S) = (n-1) / (C(n,|S|) |S| (n-|S|)) regress to the exact
    Shapley vector, here exact_ref.shapley.  1e-12 max|v|: two orders of magnitude over the 2e-15 seen at n = 10, cond(A) <= 20."""
    v = _grid_table(n, 40 + n)
    keep, w = ref.enumerated(n)
    phi = ref.estimate(keep, v[keep.astype(np.int64)], v[0], v[-1], n, w)
    want = exact_ref.shapley(v, n)
    scale = float(np.abs(v).max())
    print("n=%d: max |phi - exact| / max|v| = %.3g" % (n, np.abs(phi - want).max() / scale))
    assert np.abs(phi - want).max() <= 1e-12 * scale
    assert abs(phi.sum() - (float(v[-1]) - float(v[0]))) <= 1e-12 * scale


def test_additive_game_is_recovered_from_any_rows_with_a_regular_gram_matrix():
    """v(S) = v0 + sum of a_i over S lies in the regression's model, so any rows whose A is regular return a (the residual is
    zero whatever the weights): n = 5, the 80 paired rows of a seeded draw of 40."""
    n, s = 5, 40
    rng = np.random.default_rng(5)
    a_true, v0 = rng.standard_normal(n), 0.75
    np.random.seed(11)
    sizes, orders = ref.host_draw(n, s)
    keep = ref.rows_from_orders(orders, sizes, n)
    assert len(keep) == 2 * s
    gram, _, w = ref.moments(keep, np.zeros(len(keep)), 0.0, n)
    assert np.linalg.matrix_rank(gram / w) == n and np.linalg.cond(gram / w) < 1e3      # the seed's rows determine the regression
    v = v0 + ref.membership(keep, n) @ a_true                # float64 rewards
    phi = ref.estimate(keep, v, v0, v0 + a_true.sum(), n, gram="sampled")
    assert np.abs(phi - a_true).max() <= 1e-12 * np.abs(a_true).max()


@pytest.mark.parametrize("n", range(2, 11))
def test_analytic_gram_is_the_enumeration_weighted_gram(n):
    from interpret_quality_amd import kernelshap
    keep, w = ref.enumerated(n)
    gram, _, wsum = ref.moments(keep, np.zeros(len(keep), dtype=np.float32), 0.0, n, w)
    assert np.abs(ref.analytic_gram(n) - gram / wsum).max() <= 1e-14
    assert np.abs(kernelshap.analytic_gram(n) - gram / wsum).max() <= 1e-14
    assert np.array_equal(kernelshap.analytic_gram(n), kernelshap.analytic_gram(n).T)


def test_size_cdf_is_symmetric_ends_at_one_and_n2_draws_size_one():
    from interpret_quality_amd import kernelshap
    for n in (2, 3, 8, 33, 64):
        cdf = kernelshap.size_cdf(n)
        assert cdf.shape == (n - 1,) and cdf.dtype == np.float64 and cdf[-1] == 1.0
        assert np.array_equal(cdf, ref.size_cdf(n))
        p = np.diff(np.concatenate([[0.0], cdf]))
        assert np.abs(p - p[::-1]).max() <= 4 * n * ref.U            # p(s) = p(n - s), up to the roundings of the running sum
        assert np.all(p > 0)
    np.random.seed(3)
    assert np.all(kernelshap.draw_sizes(2, 100) == 1)
    np.random.seed(3)
    s = kernelshap.draw_sizes(7, 1000)
    assert s.min() >= 1 and s.max() <= 6 and s.dtype == np.int32
    np.random.seed(3)
    assert np.array_equal(s, ref.sizes_from_uniforms(7, np.random.random_sample(1000)))
    assert kernelshap.default_samples(8) == 9000 and kernelshap.default_samples(32) == 33000 and kernelshap.default_samples(2) == 3000
    assert kernelshap.running_counts(8, 1800) == [900, 1800]
    assert kernelshap.running_counts(2, 700, paired=True) == [300, 600] and kernelshap.running_counts(4, 1001, paired=False) == [500, 1000]
    w = kernelshap.enumeration_weights(6)
    assert w[0] == w[6] == 0 and np.array_equal(w[1:6], ref.enumerated(6)[1][[0, 2, 6, 14, 30]])      # masks 1, 3, 7, 15, 31


def test_kshap_entry_points_are_declared_bound_and_exported():
    build.build(verbose=False)
    lib = _lib.load()
    header = open(os.path.join(REPO, "include", "iq.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NAMES:
        assert name in _lib.SIGNATURES, name
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert hasattr(lib, name), name
    version = int(re.search(r"#define IQ_ABI_VERSION (\d+)", header).group(1))
    assert _lib.ABI_VERSION == lib.iq_version() == version >= 114
    # argument checks that need no device
    assert lib.iq_kshap_scratch_bytes(0, 8, 1) == 0 and lib.iq_kshap_scratch_bytes(10, 1, 1) == 0
    assert lib.iq_kshap_scratch_bytes(10, 65, 1) == 0 and lib.iq_kshap_scratch_bytes(10, 8, 0) == 0
    assert 0 < lib.iq_kshap_scratch_bytes(10, 8, 1) <= lib.iq_kshap_scratch_bytes(33000, 64, 1) < lib.iq_kshap_scratch_bytes(33000, 64, 216)
    assert lib.iq_kshap_scratch_bytes((1 << 24) - 2, 24, 1) < 64 << 20        # the chunk count is capped: an enumerated game stays small
    assert lib.iq_kshap_keep_masks(None, None, None, 4, 1, 1, None, None) == -1 and b"outside 2..64" in lib.iq_last_error()
    assert lib.iq_kshap_keep_masks(None, None, None, 0, 8, 1, None, None) == 0
    assert lib.iq_kshap_accum(None, None, None, None, 0, 8, 1, None, None, None, None, 0, None) == -1
    assert lib.iq_kshap_solve(None, None, None, None, None, 65, 1, None) == -1


def test_wrappers_refuse_cpu_tensors_and_bad_arguments():
    import torch
    from interpret_quality_amd import hip_ops, kernelshap
    with pytest.raises(_lib.IqError):
        hip_ops.kshap_keep_masks(torch.zeros((4, 8), dtype=torch.int32), torch.ones((4,), dtype=torch.int32))
    with pytest.raises(_lib.IqError):
        hip_ops.kshap_accum(torch.zeros((4,), dtype=torch.int64), torch.zeros((1, 4)), torch.zeros((1,), dtype=torch.float64), 8)
    with pytest.raises(_lib.IqError):
        hip_ops.kshap_solve(torch.eye(8, dtype=torch.float64), torch.zeros((1, 8), dtype=torch.float64), torch.zeros((1,), dtype=torch.float64))
    for n in (1, 65):
        with pytest.raises(_lib.IqError):
            kernelshap.size_cdf(n)
        with pytest.raises(_lib.IqError):
            kernelshap.analytic_gram(n)
    with pytest.raises(_lib.IqError):
        kernelshap.enumerated(25, "cpu")


def test_driver_parser_refuses_1_and_65_regions(capsys):
    from interpret_quality_amd import kernel_stage
    for bad in ("1", "65"):
        with pytest.raises(SystemExit):
            kernel_stage.make_args(["--model", "pointnet", "--num_regions", bad])
        assert "2 to 64" in capsys.readouterr().err
    args = kernel_stage.make_args(["--model", "pointnet"])
    assert args.num_regions == 32 and args.samples is None and args.gram == "sampled" and not args.unpaired and not args.compare_exact
    args = kernel_stage.make_args(["--model", "pointnet", "--num_regions", "64", "--samples", "512", "--unpaired", "--gram", "analytic"])
    assert args.num_regions == 64 and args.samples == 512 and args.unpaired and args.gram == "analytic"
    with pytest.raises(SystemExit):
        kernel_stage.make_args(["--model", "pointnet", "--num_regions", "25", "--compare_exact"])
    assert "24" in capsys.readouterr().err


def test_game_refuses_a_bad_gram_before_it_draws_or_loads_the_library(monkeypatch):
    """The mirror of test_kshap_counter_cpu.py::test_python_level_refusals_need_no_library_call for the narrow game: a ``gram``
    outside GRAMS is refused before a row is drawn (NumPy's global generator stands where it stood) and before any forward."""
    import argparse

    from interpret_quality_amd import kernelshap

    def no_library():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", no_library)
    state = np.random.get_state()
    for call in (kernelshap.game, kernelshap.shapley):
        with pytest.raises(_lib.IqError, match="gram must be one of"):
            call(None, None, None, None, argparse.Namespace(num_regions=8), samples=64, gram="bogus")
    after = np.random.get_state()
    assert state[0] == after[0] and np.array_equal(state[1], after[1]) and state[2:] == after[2:]
