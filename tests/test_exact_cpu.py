"""CPU: the exact-game entry points exist and are bound; the brute-force reference (tests/exact_ref.py) satisfies the axioms
and identities that define the quantities; and the reference-side half of the end-to-end check: the reference's sampled
estimate agrees with the brute-force exact value of its own game."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import exact_ref
from interpret_quality_amd import _lib, build, synth

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("iq_enum_keep_masks", "iq_exact_shapley", "iq_exact_interactions", "iq_moebius", "iq_exact_scratch_bytes")


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return _lib.load()


def test_exact_entry_points_are_declared_bound_and_exported(lib):
    header = open(os.path.join(REPO, "include", "iq.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NAMES:
        assert name in _lib.SIGNATURES, name
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert hasattr(lib, name), name
    from interpret_quality_amd import exact, hip_ops
    limit = int(re.search(r"#define IQ_MAX_EXACT_PLAYERS (\d+)", header).group(1))
    assert limit == 24 == hip_ops.MAX_EXACT_PLAYERS == exact.MAX_PLAYERS
    assert _lib.ABI_VERSION == lib.iq_version() >= 104


def test_host_side_argument_checks(lib):
    """What the entry points refuse before any launch (no GPU involved): a repeated player, a player inside base, n out of
    range; and the scratch size grows with n and P."""
    def enum(players, n, base):
        arr = np.asarray(players, dtype=np.int32) if players is not None else None
        return lib.iq_enum_keep_masks(None, 0, 0, ctypes.c_void_p(arr.ctypes.data if arr is not None else 0), n, base, None)
    assert enum(None, 8, 0) == 0 and enum([3, 1, 2], 3, 0b10001) == 0       # count = 0: validated, nothing launched
    assert enum([3, 1, 3], 3, 0) == -1 and b"two players" in lib.iq_last_error()
    assert enum([3, 1, 2], 3, 0b10) == -1 and b"base" in lib.iq_last_error()
    assert enum(None, 4, 0b100) == -1 and b"base" in lib.iq_last_error()
    assert enum([64], 1, 0) == -1 and enum([-1], 1, 0) == -1
    assert enum(None, 25, 0) == -1 and enum(None, 0, 0) == -1
    assert lib.iq_exact_scratch_bytes(25, 0) == 0 and lib.iq_exact_scratch_bytes(0, 0) == 0
    assert 0 < lib.iq_exact_scratch_bytes(8, 0) <= lib.iq_exact_scratch_bytes(8, 28) < lib.iq_exact_scratch_bytes(24, 276) < 64 << 20
    assert lib.iq_exact_scratch_bytes(8, 65535) > 0 and lib.iq_exact_scratch_bytes(8, 65536) == 0
    assert lib.iq_exact_interactions(None, 8, None, 65536, None, None, 0, None) == -1 and b"65535" in lib.iq_last_error()
    for fn, args in ((lib.iq_exact_shapley, (None, 25, None, None, 0, None)), (lib.iq_moebius, (None, 0, None, None)),
                     (lib.iq_exact_interactions, (None, 25, None, 1, None, None, 0, None))):
        assert fn(*args) == -1


def test_hip_wrappers_refuse_cpu_tensors_and_bad_tables():
    import torch
    from interpret_quality_amd import hip_ops
    for fn in (hip_ops.exact_shapley, hip_ops.exact_interactions, hip_ops.moebius):
        with pytest.raises(_lib.IqError):
            fn(torch.zeros(8))
    with pytest.raises(_lib.IqError):
        hip_ops.enum_keep_masks(0, 4, 2, "cpu")


def test_exact_stage_refuses_more_than_24_regions(capsys):
    from interpret_quality_amd import exact_stage
    with pytest.raises(SystemExit):
        exact_stage.make_args(["--model", "pointnet", "--num_regions", "25"])
    assert "at most 24" in capsys.readouterr().err
    assert exact_stage.make_args(["--model", "pointnet"]).num_regions == 16


def _table(n, seed):
    return (np.random.default_rng(seed).standard_normal(1 << n) * 3).astype(np.float32)


@pytest.mark.parametrize("n", range(1, 11))
def test_reference_satisfies_efficiency_moebius_identities_and_symmetry(n):
    v = _table(n, n)
    pairs = [(i, j) for i in range(n) for j in range(i + 1, n)]
    phi, bound = exact_ref.shapley(v, n, with_bound=True)
    scale = float(np.abs(v).sum())      # every quantity below is a signed combination of table entries with weights <= 1
    tol = 64 * n * exact_ref.U * scale
    # efficiency: the float32 marginals differ from exact differences by half an ulp of float32 each; in exact arithmetic the sum
    # telescopes, so allow the float32 rounding of the marginals (weights sum to n over all terms of all players)
    assert abs(phi.sum() - (float(v[-1]) - float(v[0]))) <= n * 2.0 ** -24 * 2 * float(np.abs(v).max()) + tol
    # Moebius identity 1 - in exact arithmetic on the exact differences; the float32 marginals bring the same allowance
    a, abound = exact_ref.dividends(v, n, with_bound=True)
    assert np.all(abound >= 0) and np.all(bound >= 0)
    np.testing.assert_allclose(exact_ref.shapley_from_dividends(a, n), phi, rtol=0, atol=2.0 ** -24 * 2 * float(np.abs(v).max()) + tol)
    # the dividends invert: v[c] = sum of a over the subsets of c (zeta transform)
    for c in sorted({0, 1, (1 << n) - 1, (1 << n) // 3, (1 << n) - 2} & set(range(1 << n))):
        assert abs(math.fsum(a[t] for t in range(1 << n) if t & c == t) - float(v[c])) <= tol
    # Moebius identity 2, a few contexts per pair
    rng = np.random.default_rng(100 + n)
    for i, j in pairs[:6] + pairs[-2:]:
        for c in {0, *(int(x) for x in rng.integers(0, 1 << n, size=3))}:
            c &= ~((1 << i) | (1 << j))
            assert abs(exact_ref.interaction_term_from_dividends(a, c, i, j) - exact_ref.interaction_term(v, c, i, j)) \
                <= 9 * 2.0 ** -24 * float(np.abs(v).max()) + tol
    # symmetry: renaming the players renames the values, bit for bit (the same terms in the same strata; fsum is order-free)
    perm = np.random.default_rng(200 + n).permutation(n)
    w = exact_ref.relabel(v, n, perm)
    phi_w = exact_ref.shapley(w, n)
    assert np.array_equal(phi_w[perm], phi)
    if n >= 2:
        inter = exact_ref.interactions(v, n, pairs[:4])
        inter_w = exact_ref.interactions(w, n, [(int(perm[i]), int(perm[j])) for i, j in pairs[:4]])
        assert np.array_equal(inter, inter_w)
        # order 0 of the mean interaction is the single empty context
        assert inter[0, 0] == exact_ref.interaction_term(v, 0, *pairs[0])
    if n <= 6:     # the definition by permutations: all n! of them
        np.testing.assert_allclose(exact_ref.shapley_by_permutations(v, n), phi, rtol=0, atol=tol)
    if n <= 8:     # the vectorised forms used for n = 20 are the same sums
        pv, _ = exact_ref.shapley_vectorised(v, n)
        np.testing.assert_allclose(pv, phi, rtol=0, atol=tol)
        av, _ = exact_ref.dividends_vectorised(v, n)
        np.testing.assert_allclose(av, a, rtol=0, atol=tol)
        if n >= 2:
            iv, _ = exact_ref.interactions_vectorised(v, n, pairs)
            np.testing.assert_allclose(iv, exact_ref.interactions(v, n, pairs), rtol=0, atol=tol)


def test_reference_sampled_estimate_is_within_5_standard_errors_of_its_exact_value():
    """The oracle alone (PointNet, synthetic cloud 0, R = 8 regions from its own FPS): the estimate from the 1000 permutations of
    synth.make_orders(1000, 8, seed=1) lies within 5 standard errors of the brute-force exact value for every region, at 100 and
    at 1000 samples, and its RMS error shrinks from 100 to 1000 samples.  5 is a condition, not a tolerance: a per-region
    false alarm at 5 sigma is below 1e-6."""
    r = 8
    data, lbl, rid = exact_ref.oracle_setup(r)
    v = exact_ref.oracle_value_table("pointnet", synth.to_torch(synth.pointnet_state_dict(0)), data, lbl, rid, r)
    phi = exact_ref.shapley(v, r)
    assert abs(phi.sum() - (float(v[-1]) - float(v[0]))) < 1e-5
    rows = exact_ref.sampled_rows(v, synth.make_orders(1000, r, seed=1))
    rms = {}
    for s in (100, 1000):
        est, se = rows[:s].mean(axis=0), rows[:s].std(axis=0, ddof=1) / math.sqrt(s)
        z = np.abs((est - phi) / se)
        rms[s] = float(np.sqrt(((est - phi) ** 2).mean()))
        print("samples %d: max |z| %.2f, rms error %.4f" % (s, z.max(), rms[s]))
        assert z.max() < 5, (s, z)
    assert rms[1000] < rms[100]
