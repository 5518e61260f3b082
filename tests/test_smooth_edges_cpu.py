"""CPU: what tests/test_smooth_edges_gpu.py relies on (tests/smooth_cases.py, tests/smooth_ref.py).

1. The caps of the well-posedness rule: it cannot quietly empty the GPU test.
2. The NumPy restatement of the contract (closed-form gradient) equals the float64 run of the CPU oracle (autograd) on every compared
   region of every cloud, all six (mode, objective) pairs and all three bound settings, and takes the same discrete decisions.
   The bound is first-order float64 rounding over the steps taken, u = 2^-53:
     one step moves a region by `step` along g / |g|.  Both programs form g from sums over the S points (means, variances, the norm:
     relative rounding <= S u each, a handful of them) and from orientations that two eigen-solvers return to within u / gap of
     each other, gap >= MIN_GAP (relative to l1) on a compared region; so the two steps differ by at most K u step (S + 1 / MIN_GAP),
     and storing the moved point rounds by at most u max|x| more.  Over T steps, plus the start:
         |x_restatement - x_oracle| <= (T + 1) K u (step (S + 1 / MIN_GAP) + max|x|),   K = 8 for the handful of sums.
     For S = 193, T = 303: 3e-13; the largest bound of any case is below 1e-12, seven orders under the float32 error the GPU test
     measures.  First order: a difference made by an early step is also carried, and may be stretched, by the later ones - by up to
     exp(c step sum_t 1 / sqrt((S - 1) v_t)), v_t the smallest variance the ratio reads - which is no bound at all where a
     trajectory drives that variance to zero (scattering / dec on four points).  The test does not lean on that factor; it holds
     the first-order bound everywhere, which the two float64 runs meet.
   The smoothness values follow from the positions: |d var| <= 2 sqrt(s_max / (S - 1)) |dX|_F and a ratio moves by at most
   3 |d var| / s_max, with |dX|_F <= sqrt(3 S) times the bound above and s_max >= l1 / 2 over these short trajectories.
3. The float32 oracle takes the float64 run's discrete decisions on every compared region: e_ref then measures rounding, not
   another trajectory.
4. The tightened bounds bind: under "var" every compared region detaches a variance, under "dist" every compared region stops by
   stop_ratio; under the reference's constants no compared region does either within the three epochs.
5. Power: four deliberately wrong restatements (smooth_ref.VARIANTS) are above the GPU test's bar, FACTOR e_ref + FLOOR with e_ref
   the float32 oracle's own error, on the case meant to catch each.
"""
import numpy as np
import pytest

import smooth_cases as C
import smooth_ref as SR

U = 2.0 ** -53
K = 8
CASES = [(n, m, o) for n in C.NAMES for m, o in C.PAIRS]
case_id = lambda p: "-".join(p)


def test_the_rule_keeps_the_regions_it_must():
    sizes = C.cloud("sizes")
    s = C.region_sizes(sizes)
    assert sizes.pts.shape == (1024, 3) and sizes.num_regions == 17 and sorted(s.tolist()) == sorted(C.SIZES + (0, 1, 144))
    assert C.compared(sizes) == [r for r in range(17) if s[r] >= 4] and len(C.compared(sizes)) == 13 and len(C.populated(sizes)) == 15
    assert np.abs(np.diff(sizes.rid)).max() > 1 and (np.diff(sizes.rid) != 0).mean() > 0.5            # interleaved
    one, tail, tiny, spectra = (C.cloud(n) for n in ("one", "tail", "tiny", "spectra"))
    assert one.pts.shape == (1024, 3) and C.compared(one) == [0]
    assert tail.pts.shape == (1000, 3) and C.region_sizes(tail).tolist() == [500, 300, 200] and C.compared(tail) == [0, 1, 2]
    assert tiny.pts.shape == (5, 3) and C.region_sizes(tiny).tolist() == [4, 1] and C.compared(tiny) == [0]
    assert spectra.pts.shape[0] <= 256 and spectra.labels == C.SPECTRA
    assert C.compared(spectra) == [C.SPECTRA.index("distinct")]


def test_the_spectra_are_what_their_names_say_and_their_float32_covariance_is_exact():
    c = C.cloud("spectra")
    want = {"distinct": (5 / 256, 1 / 256, 1 / 1024), "two_equal": (5 / 256, 1 / 256, 1 / 256), "isotropic": (1 / 64,) * 3,
            "plane": (5 / 256, 5 / 1024, 0.0), "line": (85 / 4096, 0.0, 0.0), "identical": (0.0, 0.0, 0.0)}
    for r, label in enumerate(c.labels):
        x = c.pts[c.rid == r]
        d = x - x.mean(axis=0, dtype=np.float32)
        cov32 = (d.T @ d / np.float32(len(x) - 1)).astype(np.float32)
        d64 = x.astype(np.float64) - x.astype(np.float64).mean(axis=0)
        assert np.array_equal(cov32.astype(np.float64), d64.T @ d64 / (len(x) - 1)), label
        assert np.array_equal(cov32, np.diag(np.diag(cov32))), label                                   # axis-aligned: entries exactly 0
        assert sorted(np.diag(cov32).tolist(), reverse=True) == list(want[label]), label


def bounds(c, run, r):
    """-> (position bound, smoothness bound) of region r after the steps ``run`` took (the derivation above)."""
    s = int(C.region_sizes(c)[r])
    steps = sum(run["trace"][r]["iters"])
    pos = (steps + 1) * K * U * (SR.DEFAULTS["step"] * (s + 1 / C.MIN_GAP) + float(np.abs(c.pts).max()))
    l1 = C.eigenvalues64(c, r)[0]
    return pos, 3 * 2 * np.sqrt(3 * s / (s - 1)) * pos / np.sqrt(l1 / 2) + 16 * U


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_restatement_equals_the_float64_oracle_and_the_float32_oracle_takes_its_decisions(case):
    name, mode, objective = case
    c = C.cloud(name)
    regions = C.compared(c)
    for which in C.SETTINGS:
        kw = C.setting(name, which)
        rs, o64, o32 = C.restatement(c, mode, objective, kw), C.oracle(c, mode, objective, kw, "float64"), C.oracle(c, mode, objective, kw)
        assert all(sum(rs["trace"][r]["iters"]) > 0 for r in regions)                                 # every compared region moved
        worst = 0.0
        for r in regions:
            pos, sm = bounds(c, rs, r)
            m = c.rid == r
            e_pos, e_sm = C.err_points(rs["data"], o64["data"], m), C.err_regions(rs["smoothness"], o64["smoothness"], [r])
            e_orig = C.err_regions(rs["orig"].T, o64["orig"].T, [r])
            worst = max(worst, e_pos / pos)
            assert e_pos <= pos and e_sm <= sm and e_orig <= sm, (which, r, e_pos, pos, e_sm, e_orig, sm)
        assert not C.trace_differences(rs["trace"], o64["trace"], regions), which
        assert C.count_difference(rs["trace"], o64["trace"], regions) == 0, which
        assert not C.trace_differences(rs["trace"], o32["trace"], regions), which
        print("%-26s %-4s restatement / oracle64: worst share of the bound %.3f; float32 oracle: e_ref %.3g, counts differ by <= %d"
              % (case_id(case), which, worst, C.err_points(o32["data"], rs["data"], C.point_mask(c, regions)),
                 C.count_difference(rs["trace"], o32["trace"], regions)))


@pytest.mark.parametrize("name", C.NAMES)
def test_the_tightened_bounds_bind_on_every_compared_region(name):
    c = C.cloud(name)
    regions = C.compared(c)
    for mode, objective in C.PAIRS:
        run = {w: C.restatement(c, mode, objective, C.setting(name, w))["trace"] for w in C.SETTINGS}
        for r in regions:
            assert C.detached(run["var"], r) and not C.stopped_by_ratio(c, run["var"], r), (mode, objective, r)
            assert C.stopped_by_ratio(c, run["dist"], r) and not C.detached(run["dist"], r), (mode, objective, r)
            assert not C.detached(run["ref"], r) and not C.stopped_by_ratio(c, run["ref"], r), (mode, objective, r)


# variant -> the case meant to catch it: (cloud, mode, objective, setting)
POWER = {"ignore_detach": ("sizes", "planarity", "inc", "var"),       # the bound must take a variance out of the gradient
         "swap_mid_min": ("sizes", "linearity", "dec", "ref"),        # linearity reads mid, not min
         "no_mean": ("tail", "scattering", "inc", "ref"),             # blobs centred away from the origin
         "biased_var": ("sizes", "planarity", "dec", "var")}          # S / (S - 1) cancels in every ratio and in g / |g|, not against
                                                                      # the absolute variance bound: 4 / 3 at S = 4


@pytest.mark.parametrize("variant", SR.VARIANTS)
def test_a_planted_error_is_above_the_bar(variant):
    name, mode, objective, which = POWER[variant]
    c = C.cloud(name)
    kw = C.setting(name, which)
    mask = C.point_mask(c, C.compared(c))
    f64 = C.restatement(c, mode, objective, kw)
    e_ref = C.err_points(C.oracle(c, mode, objective, kw)["data"], f64["data"], mask)
    e_bad = C.err_points(C.restatement(c, mode, objective, kw, variant=variant)["data"], f64["data"], mask)
    print("%-14s %s: e %.3g, e_ref %.3g, bar %.3g" % (variant, "-".join(POWER[variant]), e_bad, e_ref, C.bar(e_ref)))
    assert e_bad > C.bar(e_ref)
    # and in a single step from the input cloud, in units of step, wherever the variant changes the first step at all
    if variant in ("swap_mid_min", "no_mean"):
        one = dict(kw, epochs=1, max_iteration=0)
        f64 = C.restatement(c, mode, objective, one)
        e_ref = C.err_points(C.oracle(c, mode, objective, one)["data"], f64["data"], mask, SR.DEFAULTS["step"])
        e_bad = C.err_points(C.restatement(c, mode, objective, one, variant=variant)["data"], f64["data"], mask, SR.DEFAULTS["step"])
        assert e_bad > C.bar(e_ref), (e_bad, e_ref)
