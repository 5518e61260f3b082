"""The clouds, the well-posedness rule, the bound settings, the reference runs and the error bar behind
tests/test_smooth_edges_cpu.py and tests/test_smooth_edges_gpu.py: the smoothness enumeration (csrc/iq_smooth.hip) held to a float64
run at the region sizes and spectra where its wavefront-per-region kernel changes shape, in the manner of tests/f64_cases.py.

Clouds (seeded NumPy only; the arrays are shared and must not be written):
  sizes    N = 1024, R = 17: regions of 2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 127, 128, 129, 193 points, an empty region, a region of one
           point and a last region of the 144 points that remain; ids interleaved by a seeded permutation
  one      N = 1024, R = 1: the kernel's LDS arrays full, 16 points per lane
  tail     N = 1000, R = 3: 500 / 300 / 200 points, interleaved; the last ballot of the compaction loop is partial
  tiny     N = 5, R = 2: four points and one point; a single, partial ballot
  spectra  N = 50, R = 6: axis-aligned point sets on small dyadic coordinates with mean exactly 0 and S - 1 a power of two, so the
           float32 covariance is exact: distinct diagonal, two equal eigenvalues, isotropic, a plane z = 0, a line along x, and five
           identical points (lambda_max = 0: smoothness NaN, no step is ever entered)
A blob is standard_normal((S,3)) * scales, times a random rotation, plus a centre uniform in [-0.5, 0.5]^3.

A region is COMPARED (steps and trajectories held to the bar) when S >= 4 and the float64 eigenvalues l1 >= l2 >= l3 of its float64
covariance have l3 / l1 >= 5e-3 and both gaps >= 0.03 l1; every other region is held to invariants only (the reference itself is ill
posed there: the basis of a null or repeated eigenspace is arbitrary).  The rule reads the inputs alone.

The bar is the project's (tests/f64_cases.py): with e(x) the max over the compared regions of |x - float64| in the stated unit,
e(HIP) <= FACTOR e_ref + FLOOR, FACTOR = 4, FLOOR = 1e-7, e_ref the float32 CPU oracle's own e on the same case.

Importing this module touches no GPU.  Not collected by pytest (no test_ prefix)."""
from typing import NamedTuple

import numpy as np

import smooth_ref as SR

MODES = SR.MODES
PAIRS = [(m, o) for m in MODES for o in ("inc", "dec")]
FACTOR = 4                  # tests/f64_cases.py
FLOOR = 1e-7                # the floor of f64_cases.bar
EPOCHS = 3
MIN_POINTS, MIN_RATIO, MIN_GAP = 4, 5e-3, 0.03
BLOB = (0.10, 0.05, 0.02)
SIZES = (2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 127, 128, 129, 193)


class Cloud(NamedTuple):
    name: str
    pts: np.ndarray         # (N,3) float32
    rid: np.ndarray         # (N,) int64
    num_regions: int
    labels: tuple = ()      # spectra: the name of each region


def _rotation(rng):
    q, r = np.linalg.qr(rng.standard_normal((3, 3)))
    return q * np.sign(np.diag(r))


def _blob(rng, s, scales=BLOB):
    return rng.standard_normal((s, 3)) * np.asarray(scales) @ _rotation(rng).T + rng.uniform(-0.5, 0.5, 3)


def _interleave(rng, blocks):
    """[(S_r,3) or None] -> pts float32, rid int64, shuffled so that region ids interleave."""
    pts = np.concatenate([b for b in blocks if b is not None and len(b)])
    rid = np.concatenate([np.full(len(b), r, np.int64) for r, b in enumerate(blocks) if b is not None and len(b)])
    perm = rng.permutation(len(rid))
    return np.ascontiguousarray(pts[perm].astype(np.float32)), np.ascontiguousarray(rid[perm])


def _sizes():
    rng = np.random.default_rng(5101)
    blocks = [_blob(rng, s) for s in SIZES] + [None, _blob(rng, 1), _blob(rng, 1024 - sum(SIZES) - 1)]
    return Cloud("sizes", *_interleave(rng, blocks), 17)


def _one():
    rng = np.random.default_rng(5102)
    return Cloud("one", *_interleave(rng, [_blob(rng, 1024, (0.4, 0.2, 0.1))]), 1)


def _tail():
    rng = np.random.default_rng(5103)
    return Cloud("tail", *_interleave(rng, [_blob(rng, s) for s in (500, 300, 200)]), 3)


def _tiny():
    for seed in range(5104, 5204):                      # re-seeded until region 0 meets the rule
        rng = np.random.default_rng(seed)
        c = Cloud("tiny", *_interleave(rng, [_blob(rng, 4), _blob(rng, 1)]), 2)
        if compared(c) == [0]:
            return c
    raise AssertionError("no seed gives a well-posed region of four points")


def _axis(*per_axis):
    """Origin plus +-a on axis k for every a of per_axis[k]."""
    out = [np.zeros(3)]
    for k, vals in enumerate(per_axis):
        for a in vals:
            for s in (1.0, -1.0):
                p = np.zeros(3)
                p[k] = s * a
                out.append(p)
    return np.array(out)


SPECTRA = ("distinct", "two_equal", "isotropic", "plane", "line", "identical")


def _spectra():
    rng = np.random.default_rng(5105)
    cube = np.array([[0, 0, 0]] + [[sx, sy, sz] for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)]) * 0.125
    blocks = [_axis((0.25, 0.125), (0.125,), (0.0625,)),                   # cov diag(5/256, 1/256, 1/1024)
              _axis((0.25, 0.125), (0.125,), (0.125,)),
              cube,                                                         # cov = I / 64
              _axis((0.25, 0.125), (0.125, 0.0625), ()),
              _axis((0.25, 0.125, 0.0625, 0.03125), (), ()),
              np.tile(np.array([[0.25, -0.5, 0.125]]), (5, 1))]
    assert all(len(b) == 9 for b in blocks[:5])
    return Cloud("spectra", *_interleave(rng, blocks), 6, SPECTRA)


_BUILD = {"sizes": _sizes, "one": _one, "tail": _tail, "tiny": _tiny, "spectra": _spectra}
NAMES = tuple(_BUILD)
_CLOUDS = {}


def cloud(name):
    if name not in _CLOUDS:
        _CLOUDS[name] = _BUILD[name]()
    return _CLOUDS[name]


def region_sizes(c):
    return np.bincount(c.rid, minlength=c.num_regions)


def eigenvalues64(c, r):
    """Float64 eigenvalues, descending, of the float64 covariance of region r (S >= 2)."""
    return SR.orientations(c.pts[c.rid == r].astype(np.float64))[1]


def compared(c):
    """The regions whose steps and trajectories are held to the bar; computed from the inputs alone."""
    out = []
    for r, s in enumerate(region_sizes(c)):
        if s < MIN_POINTS:
            continue
        l1, l2, l3 = eigenvalues64(c, r)
        if l1 > 0 and l3 / l1 >= MIN_RATIO and l1 - l2 >= MIN_GAP * l1 and l2 - l3 >= MIN_GAP * l1:
            out.append(r)
    return out


def populated(c):
    """The regions of at least two points: the ones the reference can process at all."""
    return [r for r, s in enumerate(region_sizes(c)) if s >= 2]


def point_mask(c, regions):
    return np.isin(c.rid, np.asarray(regions, dtype=np.int64))


# ---- bound settings ---------------------------------------------------------------------------------------------------------

# "ref": the reference's constants, where neither bound engages in three epochs of a typical region.  "var": the variance bound
# tightened until every compared region detaches a variance; "dist": the distance bound tightened until every compared region stops by
# stop_ratio; tests/test_smooth_edges_cpu.py asserts both from the trace.  A region's step has Frobenius length `step` whatever S, so
# a point moves about step / sqrt(S) per iteration and a variance about 2 step sqrt(var / (S - 1)): the bounds that bind scale with
# the region, and the clouds of one big region or of four points get their own.
_TIGHT = {"sizes": (1e-4, 1.5e-3), "one": (1e-4, 1e-3), "tail": (1e-4, 2e-3), "tiny": (1e-4, 1e-3), "spectra": (1e-4, 2e-3)}
SETTINGS = ("ref", "var", "dist")


def setting(name, which):
    """-> the keyword overrides of smooth_ref.enumerate_regions (the oracle takes ``epoch`` for ``epochs``: ``oracle_kw``)."""
    var, dist = _TIGHT[name]
    kw = dict(epochs=EPOCHS)
    if which == "var":
        kw["var_threshold"] = var
    elif which in ("dist", "project"):
        kw["dist_threshold"] = dist
    else:
        assert which == "ref", which
    return kw


def oracle_kw(kw):
    out = dict(kw)
    out["epoch"] = out.pop("epochs")
    return out


# ---- the runs ----------------------------------------------------------------------------------------------------------------

_RUNS = {}


def _key(kw):
    return tuple(sorted(kw.items()))


def restatement(c, mode, objective, kw, dtype="float64", project=False, start=None, variant=None):
    """smooth_ref.enumerate_regions on cloud ``c``, cached.  ``start`` (N,3): the enumeration restarts from that state with the
    cloud as ``origin``."""
    key = ("restatement", c.name, mode, objective, _key(kw), dtype, project, None if start is None else start.tobytes(), variant)
    if key not in _RUNS:
        pts, origin = (c.pts, None) if start is None else (start, c.pts)
        _RUNS[key] = SR.enumerate_regions(pts, c.rid, c.num_regions, mode, objective, origin=origin, project_to_bound=project,
                                          dtype=np.dtype(dtype), variant=variant, **kw)
    return _RUNS[key]


def oracle(c, mode, objective, kw, dtype="float32", start=None):
    """oracle.ref_cpu.smoothness_enumerate in ``dtype`` on the points of the regions it can process (at least two points; regions
    never read each other's points, so the sub-cloud gives those regions' own trajectories), scattered back to the outputs of
    iq_smoothness_enum: dict data (E,N,3), smoothness (E,R), orig (R,4) as float64 arrays, trace.  A region the oracle stopped keeps
    its state, and once all have stopped the oracle ends: the remaining epochs repeat the last one, as the kernel writes them."""
    key = ("oracle", c.name, mode, objective, _key(kw), dtype, None if start is None else start.tobytes())
    if key in _RUNS:
        return _RUNS[key]
    import torch
    from oracle import ref_cpu as O
    regions = populated(c)
    keep = point_mask(c, regions)
    local = np.searchsorted(np.asarray(regions), c.rid[keep])
    tt = getattr(torch, dtype)
    data = torch.from_numpy(c.pts[keep]).to(tt)[None]
    st = None if start is None else torch.from_numpy(start[keep]).to(tt)[None]
    trace = {}
    d, s, o = O.smoothness_enumerate(data, local, len(regions), mode, objective, start=st, trace=trace, **oracle_kw(kw))
    E, p = kw["epochs"], d.shape[0]
    out = dict(data=np.repeat((c.pts if start is None else start).astype(np.float64)[None], E, axis=0),
               smoothness=np.full((E, c.num_regions), np.nan), orig=np.full((c.num_regions, 4), np.nan), trace={})
    idx = np.flatnonzero(keep)
    for e in range(E):
        out["data"][e, idx] = d[min(e, p - 1), 0]
        out["smoothness"][e, regions] = s[min(e, p - 1)]
    out["orig"][regions] = o
    for j, r in enumerate(regions):
        t = trace[j]
        out["trace"][r] = dict(iters=t["iters"] + [0] * (E - len(t["iters"])), stop=t["stop"], steps=t["steps"])
    _RUNS[key] = out
    return out


def trace_differences(a, b, regions):
    """The regions on which two traces differ in a discrete decision: the steps taken per epoch and the stop epoch (which hold the
    outcome of every target test and every stop test), the order of the variances and the detach flags of every step.  The raw
    distance count is no decision - what it decides is the stop test - and it is not compared: among hundreds of points that cross
    the bound within a few dozen steps, one lies within float32 rounding of it now and then, and the count of that one step then
    differs by one between the precisions (``count_difference``)."""
    cut = lambda t: [s[:2] for s in t["steps"]]
    return [r for r in regions if a[r]["iters"] != b[r]["iters"] or a[r]["stop"] != b[r]["stop"] or cut(a[r]) != cut(b[r])]


def count_difference(a, b, regions):
    """Largest difference of a step's distance count between two traces that take the same steps."""
    return max([abs(x[2] - y[2]) for r in regions for x, y in zip(a[r]["steps"], b[r]["steps"])], default=0)


def detached(trace, r):
    """Did region r detach a variance at any step?"""
    return any(not all(live) for _, live, _ in trace[r]["steps"])


def stopped_by_ratio(c, trace, r, stop_ratio=0.5):
    """Did region r stop on the distance count of its last step?"""
    t = trace[r]
    return t["stop"] is not None and t["steps"][-1][2] / region_sizes(c)[r] > stop_ratio


# ---- the error and the bar -----------------------------------------------------------------------------------------------------

def err_points(x, ref64, mask, unit=1.0):
    """max |x - ref64| / unit over the points ``mask`` of (..,N,3) arrays."""
    d = np.abs(np.asarray(x, dtype=np.float64) - ref64)[..., mask, :]
    return float(d.max() / unit) if d.size else 0.0


def err_regions(x, ref64, regions, unit=1.0):
    """max |x - ref64| / unit over the regions ``regions`` of (..,R) arrays; ``unit`` a scalar or one value per listed region."""
    d = np.abs(np.asarray(x, dtype=np.float64) - ref64)[..., regions] / unit
    return float(d.max()) if d.size else 0.0


def bar(e_ref, factor=FACTOR):
    return factor * e_ref + FLOOR
