"""GPU: the smoothness enumeration (csrc/iq_smooth.hip, hip_ops.smoothness_enum) against a float64 run, at the region sizes, cloud
sizes and spectra where the one-wavefront-per-region kernel changes shape (tests/smooth_cases.py: clouds ``sizes``, ``one``, ``tail``,
``tiny``, ``spectra``).  The float64 anchor is the NumPy restatement of the contract (tests/smooth_ref.py), which
tests/test_smooth_edges_cpu.py holds to the float64 run of the CPU oracle; the yardstick is the float32 CPU oracle:

    e(HIP) <= FACTOR e_ref + 1e-7,   FACTOR = 4,

e(x) the max over the COMPARED regions of a case of |x - float64| in the stated unit, e_ref the float32 oracle's own e on the same
case (tests/f64_cases.py's bar).  One id per (cloud, mode, objective); every id prints one row per measure (e_hip, e_ref, ratio, bar).

(a) orig_out of EVERY region of at least two points, ill-posed ones included: the variances against the float64 eigenvalues of the
    region's covariance, descending, in units of the largest; the smoothness against the ratio of those eigenvalues.  Both are
    basis-independent.  The region of identical points: NaN where the float32 oracle has NaN, stop_epoch == epochs, points unchanged
    bit for bit.
(b) single steps (epochs 1, max_iteration 0) from the input cloud and from the float32-rounded epoch states of the float64
    trajectory (``origin`` = the input cloud), under the reference's constants and under the tightened variance bound: the
    displacement data_out - state of the compared regions in units of `step`; stop_epoch of every region and the detach pattern
    (var_out against orig_out +- var_threshold, evaluated in float32 as the kernel does) equal the float64 trace.
(c) trajectories of three epochs under the reference's constants, the tightened variance bound, the tightened distance bound, and
    the tightened distance bound with project_to_bound: positions and smoothness values of the compared regions, absolute;
    stop_epoch equals the trace.  The reference has no working projection, so there e_ref is the float32 run of the restatement.
(d) invariants of every run, all regions: points of regions with fewer than two points are the input's bits in every epoch; every
    output is finite but the NaNs (a) names; and a region's Frobenius displacement between consecutive epochs is at most
        (max_iteration + 1) (step (1 + (S + 16) 2^-23) + 1e-8 sqrt(3 S) + sqrt(3 S) 2^-22 max|x|):
    an iteration moves the region by step g / |g|_F - of Frobenius length `step` but for the float32 rounding of |g|_F (a sum of S
    terms) and of the two operations per coordinate - or by 1e-8 in each of 3 S coordinates when |g|_F == 0; storing the moved point
    rounds each coordinate by 2^-24 |x|, the projection onto the ball around the origin point (non-expansive, the point before the
    step lies inside) by three more such roundings.
(e) region ids outside [0, R): hip_ops.smoothness_enum and smoothness_enum_wide refuse -1, R and 1 << 20 with an IqError and the
    next call works; the C entry points, which do not check, copy the row of such a point through to every epoch of data_out
    and give every region the bits it has without those points.

Which regions end up invariants-only: the regions of 2 and 3 points of ``sizes`` and every region of ``spectra`` but the one with
three distinct eigenvalues; all 13 regions of ``sizes`` with four or more points, and every region of ``one``, ``tail`` and ``tiny``
that holds more than one point, are compared.

Measured on one run of this file on an MI355X (gfx950; the 39 ids in 18 s): 360 rows, none above the bar, FACTOR 4 on every row,
no kernel arithmetic changed.  e_hip / e_ref is given over the rows whose e_ref reaches the 1e-7 floor (below it both errors are
a few ulps of a ratio near 0 or 1, the floor is the bar, and their quotient says nothing: up to 400 at e_hip 6e-8); the share of
the bar over all rows.  On most position and single-step rows the kernel's error EQUALS the float32 oracle's (ratio 1.00, share
0.25): the same float32 states, bit for bit.
  cloud    compared regions   e_hip / e_ref             worst share of the bar
  sizes    13 of 15           0.19 .. 3.26              0.70  planarity / inc, project smoothness (e_hip 4.9e-7; float32 NumPy yardstick)
  one      1 of 1             0.04 .. 1.00              0.25  positions, e_hip = e_ref = 2.5e-6 .. 2.9e-6
  tail     3 of 3             0.08 .. 1.13              0.27  planarity / inc, ref smoothness (5.4e-7 against 4.8e-7)
  tiny     1 of 1 (S >= 2)    0.43 .. 1.50              0.60  planarity / dec, ref smoothness (1.0e-7 against 1.7e-8: the floor)
  spectra  1 of 6             0.54 .. 1.03              0.59  planarity / inc, dist smoothness (6.0e-8 against 1.5e-10: the floor)
  (a) orig variances: share <= 0.24, e_hip <= 5.5e-7 of lambda_max, exactly 0 on ``spectra``; (b) single steps: e_hip <= 1.8e-4 of a
  step on ``sizes`` (one ulp of a coordinate near 0.5 is 6e-5 of a step), share <= 0.37.
"""
import ctypes

import numpy as np
import pytest
import torch

import smooth_cases as C
import smooth_ref as SR
from interpret_quality_amd import _lib, hip_ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CASES = [(n, m, o) for n in C.NAMES for m, o in C.PAIRS]
case_id = lambda p: "-".join(p)
STEP = SR.DEFAULTS["step"]
# per (case id, measure), where it is not smooth_cases.FACTOR: (factor, measured ratio, reason) - none so far
FACTORS = {}
OUTPUTS = ("data", "smoothness", "var", "orig", "stop_epoch")


def hip(c, mode, objective, kw, project=False, start=None, wide=False):
    """hip_ops.smoothness_enum on cloud ``c`` -> dict of numpy arrays."""
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    cloud, origin = (up(c.pts), None) if start is None else (up(start), up(c.pts))
    fn = hip_ops.smoothness_enum_wide if wide else hip_ops.smoothness_enum
    res = fn(cloud, hip_ops.as_i32(c.rid, DEV), c.num_regions, mode, objective, origin=origin, project_to_bound=project, **kw)
    return {k: v.cpu().numpy() for k, v in res.items()}


class Rows:
    """The rows of one id: measure, e_hip, e_ref -> printed, and judged at the end so that every row of a failing id is seen."""

    def __init__(self, tag):
        self.tag, self.above = tag, []

    def add(self, measure, e_hip, e_ref):
        bar = C.bar(e_ref, FACTORS.get((self.tag, measure), (C.FACTOR,))[0])
        ratio = e_hip / e_ref if e_ref > 0 else (0.0 if e_hip == 0 else float("inf"))
        print("%-26s %-28s e_hip %.3g  e_ref %.3g  e_hip / e_ref %.2f  (bar %.3g, share %.2f)"
              % (self.tag, measure, e_hip, e_ref, ratio, bar, e_hip / bar))
        if not e_hip <= bar:
            self.above.append("%s: e_hip %.3g above %.3g" % (measure, e_hip, bar))


def frobenius_cap(c, r, kw):
    s = int(C.region_sizes(c)[r])
    it = kw.get("max_iteration", SR.DEFAULTS["max_iteration"]) + 1
    return it * (STEP * (1 + (s + 16) * 2.0 ** -23) + 1e-8 * np.sqrt(3 * s) + np.sqrt(3 * s) * 2.0 ** -22 * float(np.abs(c.pts).max()))


def check_invariants(c, got, kw, state):
    """(d) on one run that started from ``state`` (N,3) float32."""
    sizes = C.region_sizes(c)
    nan_regions = [r for r in range(c.num_regions) if sizes[r] < 2 or C.eigenvalues64(c, r)[0] == 0]
    lone = C.point_mask(c, [r for r in range(c.num_regions) if sizes[r] < 2])
    for e in range(got["data"].shape[0]):
        assert np.array_equal(got["data"][e][lone].view(np.int32), state[lone].view(np.int32)), e
    assert np.isfinite(got["data"]).all()
    fine = [r for r in range(c.num_regions) if r not in nan_regions]
    assert np.isfinite(got["smoothness"][:, fine]).all() and np.isfinite(got["orig"][fine]).all() and np.isfinite(got["var"][:, fine]).all()
    assert np.isnan(got["smoothness"][:, nan_regions]).all() and np.isnan(got["orig"][nan_regions, 3]).all()
    assert (got["stop_epoch"][sizes < 2] == -1).all() and (got["stop_epoch"][sizes >= 2] >= 0).all()
    seq = np.concatenate([state[None], got["data"]]).astype(np.float64)
    for r in C.populated(c):
        m = c.rid == r
        moved = np.sqrt(((seq[1:, m] - seq[:-1, m]) ** 2).sum(axis=(1, 2)))
        assert moved.max() <= frobenius_cap(c, r, kw), (r, moved.max())


def check_orig(rows, c, mode, got, o32):
    """(a)"""
    lam = {r: C.eigenvalues64(c, r) for r in C.populated(c)}
    live = [r for r in lam if lam[r][0] > 0]
    want_var = np.array([lam[r] for r in live])
    unit = want_var[:, :1]
    want_sm = np.array([SR.ratio(mode, lam[r][2], lam[r][1], lam[r][0]) for r in live])
    e = lambda orig: (float((np.abs(orig[live, :3].astype(np.float64) - want_var) / unit).max()),
                      float(np.abs(orig[live, 3].astype(np.float64) - want_sm).max()))
    (hv, hs), (rv, rs) = e(got["orig"]), e(o32["orig"])
    rows.add("(a) orig variances", hv, rv)
    rows.add("(a) orig smoothness", hs, rs)
    for r in lam:
        if lam[r][0] == 0:                       # identical points
            assert np.array_equal(np.isnan(got["orig"][r]), np.isnan(o32["orig"][r])) and np.isnan(got["orig"][r, 3])
            assert np.array_equal(np.isnan(got["smoothness"][:, r]), np.isnan(o32["smoothness"][:, r]))
            assert got["stop_epoch"][r] == got["data"].shape[0]
            m = c.rid == r
            for e_ in range(got["data"].shape[0]):
                assert np.array_equal(got["data"][e_][m].view(np.int32), c.pts[m].view(np.int32))


def detach_pattern(got, vth):
    """Which variances the kernel kept in the gradient at the one step of a single-step run, from its own outputs, in float32."""
    var, var0, t = got["var"][0], got["orig"][:, :3], np.float32(vth)
    return ~((var > var0 + t) | (var < var0 - t))


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_enumeration_is_within_the_float64_bar(case):
    name, mode, objective = case
    c = C.cloud(name)
    regions = C.compared(c)
    mask = C.point_mask(c, regions)
    rows = Rows(case_id(case))
    assert regions
    # (c) trajectories, (a) on the first of them, (d) on each
    for which in C.SETTINGS + ("project",):
        kw = C.setting(name, which)
        project = which == "project"
        f64 = C.restatement(c, mode, objective, kw, project=project)
        ref = C.restatement(c, mode, objective, kw, "float32", project=True) if project else C.oracle(c, mode, objective, kw)
        assert not C.trace_differences(f64["trace"], ref["trace"], regions), which
        got = hip(c, mode, objective, kw, project=project)
        check_invariants(c, got, kw, c.pts)
        if which == "ref":
            check_orig(rows, c, mode, got, ref)
        rows.add("(c) %s positions" % which, C.err_points(got["data"], f64["data"], mask), C.err_points(ref["data"], f64["data"], mask))
        rows.add("(c) %s smoothness" % which, C.err_regions(got["smoothness"], f64["smoothness"], regions),
                 C.err_regions(ref["smoothness"], f64["smoothness"], regions))
        assert np.array_equal(got["stop_epoch"][regions], f64["stop_epoch"][regions]), (which, got["stop_epoch"], f64["stop_epoch"])
        if project:
            far = np.linalg.norm(got["data"].astype(np.float64) - c.pts.astype(np.float64)[None], axis=2)
            # a projected point is origin + dist_threshold times a unit vector: float32 rounds the factor and the unit vector
            # (a few 2^-24 relative) and each stored coordinate by 2^-24 |x|
            assert far.max() <= kw["dist_threshold"] * (1 + 2.0 ** -20) + np.sqrt(3) * 2.0 ** -23 * float(np.abs(c.pts).max())
    # (b) single steps from the input cloud and from the rounded epoch states of the float64 trajectory
    for which in ("ref", "var"):
        kw = C.setting(name, which)
        one = dict(kw, epochs=1, max_iteration=0)
        states = [c.pts] + [s.astype(np.float32) for s in C.restatement(c, mode, objective, kw)["data"]]
        e_hip = e_ref = 0.0
        for j, st in enumerate(states):
            start = None if j == 0 else st
            f64, ref = C.restatement(c, mode, objective, one, start=start), C.oracle(c, mode, objective, one, start=start)
            got = hip(c, mode, objective, one, start=start)
            check_invariants(c, got, one, st)
            st64 = st.astype(np.float64)
            e_hip = max(e_hip, C.err_points(got["data"][0].astype(np.float64) - st64, f64["data"][0] - st64, mask, STEP))
            e_ref = max(e_ref, C.err_points(ref["data"][0] - st64, f64["data"][0] - st64, mask, STEP))
            assert np.array_equal(got["stop_epoch"], f64["stop_epoch"]), (which, j)
            live = detach_pattern(got, one.get("var_threshold", SR.DEFAULTS["var_threshold"]))
            for r in regions:
                assert tuple(live[r]) == f64["trace"][r]["steps"][0][1] == ref["trace"][r]["steps"][0][1], (which, j, r)
        rows.add("(b) %s single steps" % which, e_hip, e_ref)
    assert not rows.above, rows.above


def test_wide_entry_gives_the_same_bits_on_the_sizes_cloud():
    c = C.cloud("sizes")
    kw = C.setting("sizes", "ref")
    narrow, wide = hip(c, "planarity", "dec", kw), hip(c, "planarity", "dec", kw, wide=True)
    assert narrow["stop_epoch"].max() > 0
    for k in OUTPUTS:
        assert narrow[k].shape == wide[k].shape and np.array_equal(narrow[k].view(np.int32), wide[k].view(np.int32)), k


# ---- (e) region ids ----

@pytest.mark.parametrize("entry", ["smoothness_enum", "smoothness_enum_wide"])
@pytest.mark.parametrize("bad", [-1, "R", 1 << 20])
def test_wrappers_refuse_region_ids_outside_the_range_and_the_next_call_works(entry, bad):
    c = C.cloud("tail")
    fn = getattr(hip_ops, entry)
    cloud, rid = torch.from_numpy(c.pts).to(DEV), hip_ops.as_i32(c.rid, DEV)
    kw = C.setting("tail", "dist")
    before = fn(cloud, rid, c.num_regions, "linearity", "inc", **kw)
    wrong = rid.clone()
    wrong[417] = c.num_regions if bad == "R" else bad
    with pytest.raises(_lib.IqError, match="region_id"):
        fn(cloud, wrong, c.num_regions, "linearity", "inc", **kw)
    after = fn(cloud, rid, c.num_regions, "linearity", "inc", **kw)
    for k in OUTPUTS:
        assert torch.equal(before[k].view(torch.int32), after[k].view(torch.int32)), k


@pytest.mark.parametrize("entry", ["iq_smoothness_enum", "iq_smoothness_enum_wide"])
def test_c_entry_copies_a_point_of_no_region_through(entry):
    """The C entry points do not check the ids (include/iq.h).  Three points with ids -1, R and 1 << 20: their rows of data_out are
    the cloud's in every epoch although the buffer held NaN, and every other output has the bits of the run without those points."""
    c = C.cloud("tail")
    n, r, e = c.pts.shape[0], c.num_regions, C.EPOCHS
    kw = C.setting("tail", "ref")
    rid = c.rid.copy()
    out_of_range = {5: -1, 417: r, 998: 1 << 20}
    for i, v in out_of_range.items():
        rid[i] = v
    rest = np.ones(n, bool)
    rest[list(out_of_range)] = False
    want = hip_ops.smoothness_enum(torch.from_numpy(c.pts[rest]).to(DEV), hip_ops.as_i32(rid[rest], DEV), r, "scattering", "inc", **kw)
    want = {k: v.cpu().numpy() for k, v in want.items()}

    cloud, rid_t = torch.from_numpy(c.pts).to(DEV), hip_ops.as_i32(rid, DEV)
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)
    out = {"data": nan(e, n, 3), "smoothness": nan(e, r), "var": nan(e, r, 3), "orig": nan(r, 4),
           "stop_epoch": torch.full((r,), -7, dtype=torch.int32, device=DEV)}
    d = SR.DEFAULTS
    prm = _lib.SmoothnessParams(d["step"], d["enum_step"], d["var_threshold"], d["dist_threshold"], d["stop_ratio"], e, d["max_iteration"], 0, 0)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = getattr(_lib.load(), entry)(p(cloud), ctypes.c_void_p(0), p(rid_t), n, r, hip_ops.SMOOTHNESS_MODES.index("scattering"), 1,
                                     ctypes.byref(prm), p(out["data"]), p(out["smoothness"]), p(out["var"]), p(out["orig"]),
                                     p(out["stop_epoch"]), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    got = {k: v.cpu().numpy() for k, v in out.items()}
    for i in out_of_range:
        for ep in range(e):
            assert np.array_equal(got["data"][ep, i].view(np.int32), c.pts[i].view(np.int32)), (i, ep)
    assert np.array_equal(got["data"][:, rest].view(np.int32), want["data"].view(np.int32))
    for k in OUTPUTS[1:]:
        assert np.array_equal(got[k].view(np.int32), want[k].view(np.int32)), k
    assert want["stop_epoch"].min() >= 0 and (want["data"] != c.pts[rest][None]).any()
