"""Where a coalition sits inside a large launch: the table of capped routes and the bitwise row comparison of
tests/test_launch_span_cpu.py and tests/test_launch_span_gpu.py.

The grouped families (PointNet++, PointConv, DGCNN / GCNN) evaluate up to ``max_clouds_per_call`` coalitions per launch in ONE
workspace, and at the cap that workspace is 12 to 37 GiB.  Three index widths wrap inside it (SPANS).  None of the three faults:
a buffer load past ``num_records`` returns 0 and a wrapped offset lands on another coalition's rows, so a late coalition would get
plausible, wrong logits.  The project's rule - a coalition's logits do not depend on the launch it travels in - is what
``rows_differ`` holds every row of a launch at the cap to.

Importing this module touches no GPU and does not load the library; ``routes()`` loads it (host-side size functions only).  Not
collected by pytest itself (no test_ prefix)."""
import importlib
from types import SimpleNamespace
from typing import NamedTuple

import numpy as np

import probes

GIB = 1 << 30
# name -> the first byte offset an index of that width cannot reach
SPANS = {
    "2GiB": 1 << 31,     # num_records = 0x7fffffff of every raw buffer resource in csrc/: a load behind it returns 0
    "4GiB": 1 << 32,     # a 32-bit byte offset wraps
    "8GiB": 1 << 33,     # an `int` index of floats goes negative
}

# family -> (module, model class, engine class); every class with a ``max_clouds_per_call`` (tests/test_launch_span_cpu.py scans
# the package for them).  PointNet has no cap of this kind: its step is sized by the drivers, 33 000 coalitions take 0.99 GiB.
FAMILIES = {
    "pointnet2": ("interpret_quality_amd.pointnet2", "PointNet2ClsMsg", "PointNet2Engine"),
    "pointconv": ("interpret_quality_amd.pointconv", "PointConvDensityClsSsg", "PointConvEngine"),
    "dgcnn": ("interpret_quality_amd.dgcnn", "DGCNN_cls", "DgcnnEngine"),
    "gcnn": ("interpret_quality_amd.dgcnn", "GCNN_cls", "DgcnnEngine"),
}
NARROW_REGIONS, WIDE_REGIONS, SOURCE_CLOUDS = 32, 128, 4
MAX_POINTS = 1024            # the largest cloud every coalition route takes (PointNet++ and PointConv: the compact paths stop here)
FULL_SIZE = 0.95             # see ``smallest_full_size_n``
# route -> (which size function, source clouds, regions)
ROUTES = {
    "forward_points": ("forward", 0, NARROW_REGIONS),                       # B materialised clouds through the dense forward
    "coalition_logits": ("coalition", SOURCE_CLOUDS, NARROW_REGIONS),       # PointConv: the launch builds its per-cloud tables
    "coalition_logits_cached": ("coalition", SOURCE_CLOUDS, NARROW_REGIONS),   # PointConv: tables of an earlier launch re-used
    "coalition_logits_wide": ("coalition", SOURCE_CLOUDS, WIDE_REGIONS),
    "compact": ("coalition", 1, WIDE_REGIONS),                              # wide.coalition_logits(coalitions="compact"): one cloud
}
# (family, route, twin): every route of every family, and one twin per kernel body that tests/test_f64_families_gpu.py::TWINS
# lists as different for the route - on the route that runs the most of that body (the dense forward is all grouped MLP; the
# member walk, the two-kernel contraction and the EdgeConv forms belong to the coalition entries; GCNN shares DGCNN's EdgeConv)
TABLE = (
    ("pointnet2", "forward_points", None), ("pointnet2", "forward_points", "group_fp32"),
    ("pointnet2", "coalition_logits", None), ("pointnet2", "coalition_logits", "pn2_member_walk"),
    ("pointnet2", "coalition_logits_wide", None), ("pointnet2", "compact", None),
    ("pointconv", "forward_points", None), ("pointconv", "forward_points", "group_fp32"),
    ("pointconv", "coalition_logits", None), ("pointconv", "coalition_logits", "pc_two_kernel"),
    ("pointconv", "coalition_logits_cached", None),
    ("pointconv", "coalition_logits_wide", None), ("pointconv", "compact", None),
    ("dgcnn", "forward_points", None),
    ("dgcnn", "coalition_logits", None), ("dgcnn", "coalition_logits", "edge_gemm_l2"), ("dgcnn", "coalition_logits", "edge_gemm_lds"),
    ("dgcnn", "coalition_logits_wide", None), ("dgcnn", "compact", None),
    ("gcnn", "forward_points", None), ("gcnn", "coalition_logits", None), ("gcnn", "coalition_logits_wide", None), ("gcnn", "compact", None),
)


class Route(NamedTuple):
    """One launch at the cap: ``cap`` coalitions of ``nc`` source clouds of ``n`` points over ``regions`` regions (``nc`` 0: the
    dense forward on ``cap`` materialised clouds), in a workspace of ``workspace_bytes`` that crosses the boundaries ``crosses``."""
    family: str
    route: str
    twin: str
    cap: int
    n: int
    nc: int
    regions: int
    workspace_bytes: int
    crosses: tuple

    @property
    def id(self):
        """Carries B, N and the widest boundary crossed, so a changed cap or size formula changes the id."""
        return "-".join([self.family, self.route] + ([self.twin] if self.twin else [])
                        + ["B%d" % self.cap, "N%d" % self.n, self.crosses[-1] if self.crosses else "below2GiB"])

    @property
    def bytes_per_coalition(self):
        return self.workspace_bytes / self.cap


def model_class(family):
    module, cls, _ = FAMILIES[family]
    return getattr(importlib.import_module(module), cls)


def size_fn(family, route):
    """(b, n) -> workspace bytes of ``route``: the engine class's own ``forward_bytes`` / ``coalition_bytes`` - what the launch
    allocates - on a stand-in that only carries the loaded library (an engine itself needs a GPU)."""
    from interpret_quality_amd import _lib
    module, _, eng = FAMILIES[family]
    eng = getattr(importlib.import_module(module), eng)
    me = SimpleNamespace(lib=_lib.load())
    kind, nc, _ = ROUTES[route]
    if kind == "forward":
        return lambda b, n: int(eng.forward_bytes(me, b, n))
    return lambda b, n: int(eng.coalition_bytes(me, b, nc, n))


def crossed(nbytes):
    return tuple(name for name, first in SPANS.items() if nbytes > first)


def smallest_full_size_n(family, route, cap):
    """The smallest cloud the route accepts at which a coalition's share of the workspace still has its full size: the bytes
    ONE MORE coalition adds near the cap, (bytes(cap) - bytes(cap / 2)) / (cap / 2), are at least FULL_SIZE of what they are at
    MAX_POINTS.  The per-coalition arrays are what a late coalition's offset is made of; the per-source-cloud tables at the head of
    the workspace do not move with B.  PointConv and PointNet++ size their arrays by the sampled centroids (512, 128), not by N -
    only a coalition's own point rows, under 2 %, follow N - so their smallest cloud does; DGCNN keeps N x N floats per cloud and
    needs all 1024 points.  A game of R regions needs R points."""
    need = size_fn(family, route)
    per = lambda n: (need(cap, n) - need(cap // 2, n)) / (cap - cap // 2)
    lo = max(probes.SIZE_LIMITS[family][0], ROUTES[route][2] if ROUTES[route][2] > 64 else 0)
    for n in sorted({lo, 128, 256, 512, MAX_POINTS}):
        if n >= lo and per(n) >= FULL_SIZE * per(MAX_POINTS):
            return n
    raise AssertionError((family, route))


def routes():
    """The table of (family, route[, twin]) launches that have a cap, from the model classes' ``max_clouds_per_call`` and the
    built library's size functions."""
    out = []
    for family, route, twin in TABLE:
        cap = int(model_class(family).max_clouds_per_call)
        n = smallest_full_size_n(family, route, cap)
        nbytes = size_fn(family, route)(cap, n)
        out.append(Route(family, route, twin, cap, n, ROUTES[route][1], ROUTES[route][2], nbytes, crossed(nbytes)))
    return out


def _bits(x):
    """(B,C) float32 rows of a torch tensor (any device) or an ndarray -> uint32 bits; NaNs compare by payload."""
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    x = np.ascontiguousarray(x)
    assert x.dtype == np.float32 and x.ndim == 2, (x.dtype, x.shape)
    return x.view(np.uint32)


class Positions(list):
    """The differing positions; prints as its message (empty: as [])."""
    message = ""

    def __repr__(self):
        return self.message if self else "[]"


def rows_differ(big, small_rows, bytes_per_coalition=0):
    """Positions i where row i of ``big`` (the launch at the cap) is not bit-identical to row i of ``small_rows`` (the same rows
    from small launches): a list, empty when every row agrees.  Its ``message`` (also its repr) names the first bad position, the
    byte offset position x ``bytes_per_coalition`` that a per-coalition array of that share reaches there and the boundaries of
    SPANS behind which it lies, and what the bad row looks like: all zero (a load past num_records), the bits of another
    position's reference row (a wrapped offset), or neither."""
    got, want = _bits(big), _bits(small_rows)
    assert got.shape == want.shape, (got.shape, want.shape)
    out = Positions(int(i) for i in np.flatnonzero((got != want).any(axis=1)))
    if out:
        i = out[0]
        at = int(i * bytes_per_coalition)
        same = np.flatnonzero((want == got[i]).all(axis=1))
        if not got[i].any() and want[i].any():
            looks = "is all zero"
        elif same.size:
            j = int(same[np.argmin(np.abs(same - i))])
            looks = "holds the reference row of position %d (%d rows %s)" % (j, abs(i - j), "earlier" if j < i else "later")
        else:
            cols = np.flatnonzero(got[i] != want[i])
            looks = "differs in %d of %d logits, first at logit %d: %r against %r" % (
                cols.size, got.shape[1], cols[0], got[i].view(np.float32)[cols[0]], want[i].view(np.float32)[cols[0]])
        out.message = ("%d of %d rows differ, the first at position %d = byte offset %d (%.2f GiB) at %.0f bytes per coalition, %s; "
                       "that row %s; the last bad position is %d" % (
                           len(out), got.shape[0], i, at, at / GIB, bytes_per_coalition,
                           "behind the %s boundary" % crossed(at)[-1] if crossed(at) else "below every boundary", looks, out[-1]))
    return out
