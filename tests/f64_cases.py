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

Importing this module touches no GPU.  Not collected by pytest (no test_ prefix)."""
from typing import NamedTuple

import numpy as np

import probes
import weight_variants as V

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
    the source clouds are scaled by this factor about the origin (PointNet++'s pair-table overflow, ``pn2_pair_rows``)."""
    name: str
    spec: probes.CoalitionCase
    wide: bool = False
    shrink: float = 1.0

    @property
    def id(self):
        return "%s-%s" % (self.name, self.spec.id)


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
    assert member[0].all() and not member[-1].any()
    centers = clouds.mean(axis=1, dtype=np.float32)
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
    i = inputs(case)
    rows = 0
    for c in range(case.spec.nc):
        p = np.concatenate([i["clouds"][c], i["centers"][c][None]]).astype(np.float64)
        d = ((p[:, None, :] - p[None, :, :]) ** 2).sum(-1)
        rows += int((d <= radius * radius - shave).sum())
    return rows, case.spec.nc * PN2_PAIR_FAN * (case.spec.n + 1)


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
        sd = V.variant(family, variant)
        masked = inputs(case)["masked"]
        out = {"choices": {}}
        for dt in ("float32", "float64"):
            logits, aux = V.oracle_forward(family, sd, masked, dt, return_aux=True)
            out["f" + dt[-2:]] = logits.double().numpy()
            out["choices"][dt] = _choices(family, aux, masked, dt)
        out["e_ref"] = rel_err(out["f32"], out["f64"])
        out["bar"] = bar(out["e_ref"])
        _RUNS[key] = out
    return _RUNS[key]


def choice_mismatches(run):
    """Names of the discrete choices on which the float32 and the float64 run differ."""
    a, b = run["choices"]["float32"], run["choices"]["float64"]
    assert [n for n, _ in a] == [n for n, _ in b]
    return [n for (n, x), (_, y) in zip(a, b) if x.shape != y.shape or not np.array_equal(x, y)]


def rel_err(x, ref64):
    return float(np.abs(np.asarray(x, dtype=np.float64) - ref64).max() / np.abs(ref64).max())


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
