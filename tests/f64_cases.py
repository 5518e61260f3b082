"""The cases, the two oracle runs and the error bar behind tests/test_f64_families_cpu.py and tests/test_f64_families_gpu.py: PointNet++,
PointConv and GCNN held to a float64 run of the CPU oracle, the way tests/test_stress_weights_gpu.py (a) holds PointNet.

With e(x) = max |x - float64| / max |float64|, a route of the HIP path passes when e(route) <= bar(e_ref) = min(FACTOR e_ref + 1e-7,
1e-4), e_ref the float32 CPU oracle's own error on the same clouds and weights: the float32 oracle measures how hard the case is,
FACTOR = 4 (the PointNet test's figure) allows for another summation order.

The masked clouds are built HERE, on the host (numpy: kept rows copied, masked rows set to the centre), from a centre computed
once in float32, so the CPU test and the GPU test see the same bytes; the GPU test shows that iq_mask_coalitions with that centre
writes the same bytes.

The bar means something only while the float32 and the float64 oracle make the same discrete choices (FPS centroids, ball-query
groups, kNN lists) - otherwise e_ref measures another network, not rounding.  ``oracle_run`` records every such choice of both runs;
tests/test_f64_families_cpu.py asserts that they agree for every (case, variant) of ``PAIRS``.

``POSED_PAIRS`` are the same clouds at the ends of the pose sweeps' grids (``POSES``: the constants of pose_sweep.py), posed in
numpy float32 and masked with the centre of the POSED cloud, and a ``sweep`` case per family - one cloud under eight poses in one
launch; tests/test_pose_f64_cpu.py and tests/test_pose_f64_gpu.py run them.

Importing this module touches no GPU.  Not collected by pytest (no test_ prefix)."""
from typing import NamedTuple

import numpy as np

import probes
import weight_variants as V
from probes import rel_err  # noqa: F401  (the tests that import this module read it as F.rel_err)

FAMILIES = ("pointnet2", "pointconv", "gcnn")
VARIANTS = ("base", "seed1", "dead", "negshift", "varspread")
FACTOR = 4                # tests/test_stress_weights_gpu.py (a)
CLAMP = 1e-4              # probes.COALITION_RTOL: no bar is ever looser than what the suite held before
# the stress size of tests/test_stress_weights_gpu.py, the family's smallest cloud, one kernel-shape boundary (PointNet++: one point
# more than sa1's 512 centroids; PointConv: one fewer, so sa1's sampling repeats index 0; GCNN: one row over a 32-row pad)
SIZES = {"pointnet2": (160, 128, 513), "pointconv": (100, 64, 511), "gcnn": (40, 21, 33)}
PN2_PAIR_FAN = 192        # csrc/iq_pointnet2.hip kPairFan: sa1's pair tables hold 192 (N + 1) rows per source cloud and scale


class Case(NamedTuple):
    """``spec``: sizes and seed (probes.CoalitionCase).  ``wide``: keep rows of ceil(R / 64) words instead of one mask.  ``shrink``:
    the source clouds are scaled by this factor about the origin (PointNet++'s pair-table overflow, ``pn2_pair_rows``).  ``pose``:
    a name of ``POSES`` applied to the source clouds after ``shrink``, or "sweep": ``spec.nc`` = 8 copies of ONE source cloud under
    ``SWEEP_POSES``, sharing one region-id row and ``spec.b`` / 8 keep masks (the launch of pose_sweep.shapley_over_poses)."""
    name: str
    spec: probes.CoalitionCase
    wide: bool = False
    shrink: float = 1.0
    pose: str = None

    @property
    def id(self):
        if self.pose is None:
            return "%s-%s" % (self.name, self.spec.id)
        return "%s-%s-%s" % (self.name, self.pose, self.spec.id)


def cases(family):
    stress, smallest, edge = SIZES[family]
    seed = 7000 + 100 * FAMILIES.index(family)
    cc = lambda n, r, nc, b, k: probes.CoalitionCase(family, n, r, nc, b, seed + k)
    out = [Case("stress", cc(stress, 8, 2, 8, 0)), Case("min", cc(smallest, 8, 1, 4, 1)), Case("edge", cc(edge, 8, 1, 3, 2)),
           Case("n1024", cc(1024, 32, 1, 2, 3)), Case("wide", cc(stress, 128, 2, 8, 4), wide=True)]
    if family == "gcnn":
        out.append(Case("walk", cc(stress, 8, 1, 8, 5)))                     # nc * 8 <= b: the layer-1 graph from the neighbour-list walk
    if family == "pointconv":
        out.append(Case("nc9", cc(smallest, 8, 9, 12, 5)))                   # more than 8 source clouds: no sa1 pair tables
    if family == "pointnet2":
        # every point within 0.4 of every other: (N + 1)^2 pair rows > 192 (N + 1), sa1's widest scale falls back to the grouped MLP
        out.append(Case("overflow", cc(256, 8, 1, 4, 6), shrink=0.15))
    return out


def pairs(family):
    """[(case, variant)]: every variant on the stress size, ``base`` elsewhere."""
    return [(c, v) for c in cases(family) for v in (VARIANTS if c.name == "stress" else ("base",))]


PAIRS = [(f, c, v) for f in FAMILIES for c, v in pairs(f)]


# ---- poses: the ends of the sweeps' grids (interpret_quality_amd/pose_sweep.py) --------------------------------------------------

TRANS_NORM = 0.5          # pose_sweep.TRANS_DIST_THRESHOLD
ANGLE = np.pi / 4         # pose_sweep.ANGLE_THRESHOLD
# name -> (kind, parameter): scale factor; translation DIRECTION (made a vector of norm TRANS_NORM, what generate_trans_vector
# makes of a grid point outside the ball); rotation angles about x, y, z
POSES = {
    "s0.5": ("scale", 0.5),                     # pose_sweep.SCALE_LOWER
    "s2.0": ("scale", 2.0),                     # pose_sweep.SCALE_UPPER
    "t+": ("trans", (1.0, 1.0, 1.0)),           # a corner of the translation grid
    "t-": ("trans", (-0.5, 0.1, 0.1)),
    "r+": ("rot", (ANGLE, ANGLE, ANGLE)),
    "r-": ("rot", (-ANGLE, ANGLE, -ANGLE)),
    "id": ("scale", 1.0),
    "s1.25": ("scale", 1.25),
}
SWEEP_POSES = ("s0.5", "s2.0", "t+", "t-", "r+", "r-", "id", "s1.25")
POSED = ("s0.5", "s2.0", "t+", "r+", "r-")      # on the stress, min and edge sizes
POSED_1024 = ("s0.5", "s2.0", "t+")


def trans_vector(direction):
    """The float32 vector of norm TRANS_NORM along ``direction``, rounded as generate_trans_vector rounds it (v / |v| * threshold
    in float32)."""
    v = np.asarray(direction, dtype=np.float32)
    return (v / np.sqrt((v * v).sum(dtype=np.float32)) * np.float32(TRANS_NORM)).astype(np.float32)


def rotation(angles):
    """R = Rx.Ry.Rz of pose_sweep.rotate_xyz as a float32 (3,3) matrix: float32 sines and cosines, float32 products."""
    tx, ty, tz = (np.float32(a) for a in angles)
    cx, cy, cz = np.cos(tx), np.cos(ty), np.cos(tz)
    sx, sy, sz = np.sin(tx), np.sin(ty), np.sin(tz)
    one, zero = np.float32(1), np.float32(0)
    rx = np.array([[one, zero, zero], [zero, cx, -sx], [zero, sx, cx]], dtype=np.float32)
    ry = np.array([[cy, zero, sy], [zero, one, zero], [-sy, zero, cy]], dtype=np.float32)
    rz = np.array([[cz, -sz, zero], [sz, cz, zero], [zero, zero, one]], dtype=np.float32)
    return ((rx @ ry).astype(np.float32) @ rz).astype(np.float32)


def apply_pose(clouds, pose):
    """clouds (..., N, 3) float32 under ``pose`` (a name of POSES), in numpy float32: x * s, x + t, x . R^T."""
    kind, par = POSES[pose]
    clouds = np.asarray(clouds, dtype=np.float32)
    if kind == "scale":
        return (clouds * np.float32(par)).astype(np.float32)
    if kind == "trans":
        return (clouds + trans_vector(par)).astype(np.float32)
    return np.matmul(clouds, rotation(par).T).astype(np.float32)


def posed_cases(family):
    """The cases of ``cases(family)`` under the ends of the sweeps' grids, and the ``sweep`` case."""
    by_name = {c.name: c for c in cases(family)}
    out = [by_name[n]._replace(pose=p) for n in ("stress", "min", "edge") for p in POSED]
    out += [by_name["n1024"]._replace(pose=p) for p in POSED_1024]
    s = by_name["stress"].spec
    out.append(Case("sweep", probes.CoalitionCase(family, s.n, s.r, len(SWEEP_POSES), 4 * len(SWEEP_POSES), s.seed + 7), pose="sweep"))
    return out


def posed_pairs(family):
    """[(case, variant)]: base weights; PointConv's stress size at scale 2.0, where the float32 reference is hardest, under every
    variant."""
    out = []
    for c in posed_cases(family):
        every = family == "pointconv" and c.name == "stress" and c.pose == "s2.0"
        out += [(c, v) for v in (VARIANTS if every else ("base",))]
    return out


POSED_PAIRS = [(f, c, v) for f in FAMILIES for c, v in posed_pairs(f)]


def pair_id(p):
    return "%s-%s" % (p[1].id, p[2])


def stress_base(family):
    return cases(family)[0]


# ---- host inputs --------------------------------------------------------------------------------------------------------------

_INPUTS = {}


def inputs(case):
    """-> dict: clouds (nc,N,3) f32, centers (nc,3) f32, rid (nc,N) i32, cloud_of (b,) i32, member (b,R) bool (row 0 the full
    coalition, the last row the empty one), keep (b Python ints, or (b,W) uint64 rows when ``case.wide``), kept (b,N) bool,
    masked (b,N,3) f32.  Built once per case; the arrays are shared and must not be written."""
    if case in _INPUTS:
        return _INPUTS[case]
    s = case.spec
    if case.wide:
        from interpret_quality_amd import synth
        rng = np.random.default_rng(s.seed)
        clouds = np.stack([synth.make_cloud(int(rng.integers(0, 1000)), num_points=s.n)[0] for _ in range(s.nc)])
        rid = rng.integers(0, s.r, size=(s.nc, s.n)).astype(np.int32)
        member = rng.random((s.b, s.r)) < np.linspace(0.9, 0.1, s.b)[:, None]
        member[0], member[-1] = True, False
        cloud_of = rng.integers(0, s.nc, size=s.b).astype(np.int32)
        bit = np.left_shift(np.uint64(1), (np.arange(s.r) & 63).astype(np.uint64))
        keep = np.stack([np.where(member[:, 64 * w:64 * w + 64], bit[64 * w:64 * w + 64], np.uint64(0)).sum(axis=1, dtype=np.uint64)
                         for w in range((s.r + 63) // 64)], axis=1)
    else:
        clouds, rid, keep, cloud_of = probes.coalition_inputs(s)
        member = np.array([[(k >> j) & 1 for j in range(s.r)] for k in keep], dtype=bool)
    clouds = (clouds * np.float32(case.shrink)).astype(np.float32)
    if case.pose == "sweep":        # one source cloud, one region-id row and b / nc keep masks under every pose of SWEEP_POSES
        per = s.b // s.nc
        assert s.nc == len(SWEEP_POSES) and per * s.nc == s.b and not case.wide
        clouds = np.stack([apply_pose(clouds[0], p) for p in SWEEP_POSES])
        rid = np.repeat(rid[:1], s.nc, axis=0)
        keep = (keep[:per - 1] + [0]) * s.nc
        member = np.array([[(k >> j) & 1 for j in range(s.r)] for k in keep], dtype=bool)
        cloud_of = np.repeat(np.arange(s.nc, dtype=np.int32), per)
    elif case.pose is not None:
        clouds = apply_pose(clouds, case.pose)
    assert member[0].all() and not member[-1].any()
    centers = clouds.mean(axis=1, dtype=np.float32)       # of the POSED cloud, as pose_sweep.shapley_over_poses takes it
    kept = member[np.arange(s.b)[:, None], rid[cloud_of]]
    masked = np.where(kept[:, :, None], clouds[cloud_of], centers[cloud_of][:, None, :]).astype(np.float32)
    out = dict(clouds=clouds, centers=centers, rid=rid, cloud_of=cloud_of, member=member, keep=keep, kept=kept, masked=masked)
    _INPUTS[case] = out
    return out


def pn2_pair_rows(case, radius=0.4, shave=1e-5):
    """-> (pair rows of sa1's widest scale counted in float64 with the squared radius shaved by ``shave``, the table's capacity):
    ordered pairs (p, q) of the N source points and the centre, p = q included, within ``radius`` - what pt_count_kernel counts
    (csrc/iq_pointnet2.hip).  The float32 expanded-form distance of the kernel is within 1e-6 of the exact one on these clouds, so a
    pair counted here is a pair the kernel counts."""
    i = case if isinstance(case, dict) else inputs(case)      # posed cases: the posed clouds and their centres
    nc, n = i["clouds"].shape[:2]
    rows = 0
    for c in range(nc):
        p = np.concatenate([i["clouds"][c], i["centers"][c][None]]).astype(np.float64)
        for lo in range(0, n + 1, 256):
            d = ((p[lo:lo + 256, None, :] - p[None, :, :]) ** 2).sum(-1)
            rows += int((d <= radius * radius - shave).sum())
    return rows, nc * PN2_PAIR_FAN * (n + 1)


def pn2_side(case):
    """"fits" / "overflows": the side of the pair table's capacity that BOTH shaved counts of ``pn2_pair_rows`` put sa1's widest
    scale on, "between" when they disagree (a case that may not be used: the kernel's float32 count could go either way)."""
    tight, cap = pn2_pair_rows(case)
    loose, _ = pn2_pair_rows(case, shave=-1e-5)
    assert tight <= loose
    return "fits" if loose <= cap else "overflows" if tight > cap else "between"


# Two PointNet++ launches of two source clouds that cross the pair table's capacity (tests/test_pose_f64_*.py): cloud A as drawn,
# cloud B the same points scaled by 0.15, four coalitions each.  N = 256: alone A fits and B overflows, together they fit.  N = 400:
# alone A fits and B overflows, together they overflow.
CAPACITY_N = (256, 400)
CAPACITY_SHRINK = 0.15


def capacity_inputs(n, which):
    """``which``: "A", "B" or "AB" -> the dict of ``inputs`` (clouds, centers, rid, cloud_of, keep, kept, masked) of that launch.  A
    cloud's rows are the same bytes in its own launch and in "AB", where A's four coalitions come first."""
    key = ("capacity", n, which)
    if key not in _INPUTS:
        s = probes.CoalitionCase("pointnet2", n, 8, 1, 4, 7900 + n)
        cloud, rid, keep, _ = probes.coalition_inputs(s)
        both = np.concatenate([cloud, (cloud * np.float32(CAPACITY_SHRINK)).astype(np.float32)])
        sel = {"A": [0], "B": [1], "AB": [0, 1]}[which]
        clouds = np.ascontiguousarray(both[sel])
        rid = np.repeat(rid, len(sel), axis=0)
        cloud_of = np.repeat(np.arange(len(sel), dtype=np.int32), 4)
        keep = list(keep) * len(sel)
        member = np.array([[(k >> j) & 1 for j in range(s.r)] for k in keep], dtype=bool)
        centers = clouds.mean(axis=1, dtype=np.float32)
        kept = member[np.arange(len(keep))[:, None], rid[cloud_of]]
        masked = np.where(kept[:, :, None], clouds[cloud_of], centers[cloud_of][:, None, :]).astype(np.float32)
        _INPUTS[key] = dict(clouds=clouds, centers=centers, rid=rid, cloud_of=cloud_of, member=member, keep=keep, kept=kept, masked=masked)
    return _INPUTS[key]


# ---- the two oracle runs --------------------------------------------------------------------------------------------------------

def _choices(family, aux, masked, dtype):
    """The discrete choices of one oracle run as a list of (name, int array)."""
    if family == "pointnet2":
        out = []
        for sa in ("sa1", "sa2"):
            out.append((sa + " fps", aux[sa]["fps"].numpy()))
            out += [("%s ball query %d" % (sa, j), g.numpy()) for j, g in enumerate(aux[sa]["group_idx"])]
        return out
    if family == "pointconv":       # knn_point returns its rows unsorted: the sets
        return [(sa + " " + k, aux[sa][k].numpy() if k == "fps" else np.sort(aux[sa][k].numpy(), axis=-1))
                for sa in ("sa1", "sa2") for k in ("fps", "knn")]
    import torch
    from oracle import ref_cpu as O
    x = torch.as_tensor(masked).to(getattr(torch, dtype)).permute(0, 2, 1).contiguous()
    return [("xyz kNN", np.sort(O.knn(x, 20).numpy(), axis=-1))]


_RUNS = {}


def oracle_run(family, case, variant):
    """-> dict: f32, f64 (the logits, float64 arrays (b,10)), e_ref, bar, choices {"float32" / "float64": [(name, array)]}.
    Computed once per (case, variant)."""
    key = (case, variant)
    if key not in _RUNS:
        _RUNS[key] = run_masked(family, variant, inputs(case)["masked"])
    return _RUNS[key]


def run_masked(family, variant, masked):
    """``oracle_run`` on any (b,N,3) float32 clouds; not cached."""
    sd = V.variant(family, variant)
    out = {"choices": {}}
    for dt in ("float32", "float64"):
        logits, aux = V.oracle_forward(family, sd, masked, dt, return_aux=True)
        out["f" + dt[-2:]] = logits.double().numpy()
        out["choices"][dt] = _choices(family, aux, masked, dt)
    out["e_ref"] = rel_err(out["f32"], out["f64"])
    out["bar"] = bar(out["e_ref"])
    return out


def choice_mismatches(run):
    """Names of the discrete choices on which the float32 and the float64 run differ."""
    a, b = run["choices"]["float32"], run["choices"]["float64"]
    assert [n for n, _ in a] == [n for n, _ in b]
    return [n for (n, x), (_, y) in zip(a, b) if x.shape != y.shape or not np.array_equal(x, y)]


def bar(e_ref, factor=FACTOR):
    return min(factor * e_ref + 1e-7, CLAMP)


# ---- weights with two bf16 terms instead of three --------------------------------------------------------------------------

# the layers that run as three bf16 terms on the matrix pipe: the grouped (per-point) ones and the heads through launch_linear
BF16_GROUP_LAYERS = {
    "pointnet2": ["sa2.conv_blocks.%d.%d.weight" % (i, j) for i in (1, 2) for j in (1, 2)],      # the 128-128-256 scales, layers 2-3
    "pointconv": ["sa2.mlp_convs.1.weight", "sa2.mlp_convs.2.weight"],
    "gcnn": ["conv5.0.weight"],
}
BF16_HEAD_LAYERS = {
    "pointnet2": ["fc1.weight", "fc2.weight"],
    "pointconv": ["fc1.weight", "fc2.weight"],
    "gcnn": ["linear1.weight", "linear2.weight"],
}


def trunc16(sd, keys):
    """A copy of the numpy state dict with the weights ``keys`` rounded to 16 significant bits (to nearest, ties to even): what
    two bf16 terms hold of a float32, i.e. a product on the bf16 pipe that lost its third term."""
    out = {k: np.array(v, copy=True) for k, v in sd.items()}
    for k in keys:
        w = out[k]
        assert w.dtype == np.float32, k
        bits = w.view(np.uint32).astype(np.uint64)
        bits = (bits + 0x7F + ((bits >> 8) & 1)) & ~np.uint64(0xFF)
        out[k] = bits.astype(np.uint32).view(np.float32).reshape(w.shape)
        assert np.abs(out[k] - w).max() <= np.abs(w).max() * 2.0 ** -16 and (out[k] != w).any(), k
    return out
