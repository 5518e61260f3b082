"""CPU: the wide regression (KernelSHAP) estimator - the NumPy restatement (tests/wide_kernelshap_ref.py) against the identities
that define it (closed form = KKT solve, the enumeration identity), the host-side pieces of
interpret_quality_amd/wide_kernelshap.py, and the plumbing: entry points declared, bound and exported at ABI 115, the driver's
parser, the refusal of the sampled Gram matrix."""
import os
import re

import numpy as np
import pytest

import exact_ref
import wide_kernelshap_ref as ref
from interpret_quality_amd import _lib, build, hip_ops, wide_kernelshap

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("iq_kshap_keep_masks_wide", "iq_kshap_scratch_bytes_wide", "iq_kshap_moment_wide", "iq_kshap_phi_analytic")


@pytest.mark.parametrize("r", [2, 3, 65, 128, 1024])
def test_closed_form_is_the_kkt_solve_with_the_analytic_gram(r):
    """phi = 2 H (b - mean(b)) + delta / R against numpy.linalg.solve on [[A, 1], [1^T, 0]], A = alpha I + c 1 1^T written out:
    within R cond(A) 2^-52 max|phi|, cond(A) from the formula of DESIGN.md 5f (6665 at R = 1024)."""
    rng = np.random.default_rng(r)
    for trial in range(3):
        b, delta = rng.standard_normal(r), float(rng.standard_normal())
        closed = ref.closed_form(b, 1.0, delta, r).astype(np.float64)
        solved = ref.kkt(b, 1.0, delta, r)
        scale = float(np.abs(closed).max())
        bound = r * ref.cond_analytic(r) * 2.0 ** -52 * scale
        print("R=%d: max |closed - kkt| = %.3g, bound %.3g, cond(A) = %.4g" % (r, np.abs(closed - solved).max(), bound, ref.cond_analytic(r)))
        assert np.abs(closed - solved).max() <= bound
        assert abs(float(ref.closed_form(b, 1.0, delta, r).sum()) - delta) <= r * 2.0 ** -52 * float(np.abs(closed).sum())


def _grid_table(n, seed):
    """A random float32 table on the grid 2^-10 (tests/test_kernelshap_cpu.py): its float32 marginals are exact."""
    return (np.round(np.random.default_rng(seed).standard_normal(1 << n) * 1024) / 1024).astype(np.float32)


@pytest.mark.parametrize("n", [2, 3, 10])
def test_enumerated_rows_give_the_exact_shapley_vector_through_the_closed_form(n):
    v = _grid_table(n, 70 + n)
    keep, w = ref.enumerated(n)
    assert keep.shape == ((1 << n) - 2, 1)
    phi = ref.estimate(keep, v[keep[:, 0].astype(np.int64)], v[0], v[-1], n, w)
    want = exact_ref.shapley(v, n)
    scale = float(np.abs(v).max())
    print("n=%d: max |phi - exact| / max|v| = %.3g" % (n, np.abs(phi - want).max() / scale))
    assert np.abs(phi - want).max() <= 1e-12 * scale
    assert abs(phi.sum() - (float(v[-1]) - float(v[0]))) <= 1e-12 * scale


def test_restatement_rows_are_the_narrow_restatements_at_64_regions_and_fewer():
    rng = np.random.default_rng(9)
    for r in (2, 63, 64):
        orders = np.stack([rng.permutation(r) for _ in range(9)])
        sizes = rng.integers(1, r, size=9)
        for paired in (True, False):
            wide_rows = ref.rows_from_orders(orders, sizes, r, paired)
            assert wide_rows.shape[1] == 1 and np.array_equal(wide_rows[:, 0], ref.narrow.rows_from_orders(orders, sizes, r, paired))
        assert np.array_equal(ref.membership(wide_rows, r), ref.narrow.membership(wide_rows[:, 0], r))
    rows = ref.rows_from_orders(np.arange(130)[None], [129], 130)
    assert rows.shape == (2, 3) and rows[0, 2] == 1 and rows[1, 2] == 2 and rows[1, 0] == 0 and rows[0, 0] == 2 ** 64 - 1
    z = ref.membership(rows, 130)
    assert z.shape == (2, 130) and z[0].sum() == 129 and z[1].sum() == 1 and z[1, 129] == 1


def test_size_cdf_ends_at_exactly_one_and_is_symmetric():
    for r in (2, 65, 128, 1023, 1024):
        cdf = wide_kernelshap.size_cdf(r)
        assert cdf.shape == (r - 1,) and cdf.dtype == np.float64 and cdf[-1] == 1.0
        assert np.array_equal(cdf, ref.size_cdf(r))
        p = np.diff(np.concatenate([[0.0], cdf]))
        assert np.abs(p - p[::-1]).max() <= 4 * r * ref.U            # p(s) = p(R - s), up to the roundings of the running sum
        assert np.all(p > 0)
    np.random.seed(3)
    s = wide_kernelshap.draw_sizes(1024, 2000)
    np.random.seed(3)
    assert np.array_equal(s, ref.sizes_from_uniforms(1024, np.random.random_sample(2000)))
    assert s.dtype == np.int32 and s.min() >= 1 and s.max() <= 1023
    for bad in (1, 1025):
        with pytest.raises(_lib.IqError):
            wide_kernelshap.size_cdf(bad)
    assert wide_kernelshap.default_samples(1024) == 1025000 and wide_kernelshap.default_samples(128) == 129000
    assert wide_kernelshap.running_counts(128, 30000) == [12900, 25800]
    assert wide_kernelshap.running_counts(65, 400) == [] and wide_kernelshap.running_counts(65, 13200) == [6600, 13200]


def test_driver_parser_refuses_64_and_1025_regions(capsys):
    from interpret_quality_amd import wide_kernel_stage
    for bad in ("64", "1025", "2"):
        with pytest.raises(SystemExit):
            wide_kernel_stage.make_args(["--model", "pointnet", "--num_regions", bad])
        err = capsys.readouterr().err
        assert "65 .. 1024" in err and "final_kernel_shapley.py" in err
    args = wide_kernel_stage.make_args(["--model", "pointnet"])
    assert args.num_regions == 128 and args.samples is None and not args.unpaired and args.coalitions is None
    args = wide_kernel_stage.make_args(["--model", "pointnet2", "--num_regions", "1024", "--samples", "400", "--unpaired", "--coalitions", "compact"])
    assert args.num_regions == 1024 and args.samples == 400 and args.unpaired and args.coalitions == "compact"
    with pytest.raises(SystemExit):
        wide_kernel_stage.make_args(["--model", "pointnet", "--samples", "1"])


def test_wide_path_refuses_the_sampled_gram_and_says_why():
    for call in (lambda: wide_kernelshap.estimate(None, None, 0.0, 1.0, 128, gram="sampled"),
                 lambda: wide_kernelshap.running_estimates(None, None, 0.0, 1.0, 128, [10], gram="sampled")):
        with pytest.raises(_lib.IqError, match="factorisation") as e:
            call()
        assert "analytic" in str(e.value) and "64 regions" in str(e.value)
    with pytest.raises(_lib.IqError, match="gram must be"):
        wide_kernelshap.estimate(None, None, 0.0, 1.0, 128, gram="other")
    with pytest.raises(_lib.IqError, match="limit of 24"):
        wide_kernelshap.enumerated(25, "cpu")


def test_wide_kshap_entry_points_are_declared_bound_and_exported_at_abi_115():
    build.build(verbose=False)
    lib = _lib.load()
    header = open(os.path.join(REPO, "include", "iq.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NAMES:
        assert name in _lib.SIGNATURES, name
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert hasattr(lib, name), name
    version = int(re.search(r"#define IQ_ABI_VERSION (\d+)", header).group(1))
    assert _lib.ABI_VERSION == lib.iq_version() == version >= 115
    limit = int(re.search(r"#define IQ_MAX_WIDE_REGIONS (\d+)", header).group(1))
    assert limit == hip_ops.MAX_WIDE_REGIONS == wide_kernelshap.MAX_REGIONS == 1024
    # argument checks that need no device
    sb = lib.iq_kshap_scratch_bytes_wide
    assert sb(0, 128, 1) == 0 and sb(10, 1, 1) == 0 and sb(10, 1025, 1) == 0 and sb(10, 128, 0) == 0
    assert 0 < sb(10, 128, 1) <= sb(1025000, 1024, 1) < sb(1025000, 1024, 3)
    assert sb(1025000, 1024, 1) < 4 << 20                           # at most 256 chunks of R doubles per game
    assert lib.iq_kshap_keep_masks_wide(None, None, None, 4, 1, 1, None, None) == -1 and b"outside 2..1024" in lib.iq_last_error()
    assert lib.iq_kshap_keep_masks_wide(None, None, None, 4, 1025, 1, None, None) == -1
    assert lib.iq_kshap_keep_masks_wide(None, None, None, 0, 128, 1, None, None) == 0
    assert lib.iq_kshap_moment_wide(None, None, None, None, 0, 128, 1, None, None, None, 0, None) == -1
    assert lib.iq_kshap_phi_analytic(None, None, None, None, 1025, 1, None) == -1
    assert lib.iq_kshap_phi_analytic(None, None, None, None, 128, 1, None) == -1 and b"null pointer" in lib.iq_last_error()


def test_wide_wrappers_refuse_cpu_tensors_and_bad_shapes():
    import torch
    with pytest.raises(_lib.IqError):
        hip_ops.kshap_keep_masks_wide(torch.zeros((4, 128), dtype=torch.int32), torch.ones((4,), dtype=torch.int32))
    with pytest.raises(_lib.IqError):
        hip_ops.kshap_moment_wide(torch.zeros((4, 2), dtype=torch.int64), torch.zeros((1, 4)), torch.zeros((1,), dtype=torch.float64), 128)
    with pytest.raises(_lib.IqError, match=r"\(B, 2\)"):
        hip_ops.kshap_moment_wide(torch.zeros((4, 1), dtype=torch.int64), torch.zeros((1, 4)), torch.zeros((1,), dtype=torch.float64), 128)
    with pytest.raises(_lib.IqError):
        hip_ops.kshap_phi_analytic(torch.zeros((1, 128), dtype=torch.float64), torch.ones((1,), dtype=torch.float64),
                                   torch.zeros((1,), dtype=torch.float64))
    with pytest.raises(_lib.IqError):
        hip_ops.kshap_regions_wide(1)
