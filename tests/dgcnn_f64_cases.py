"""The cases behind tests/test_dgcnn_f64_cpu.py and tests/test_dgcnn_f64_gpu.py: DGCNN held to a float64 run of the CPU oracle at the
bar of tests/f64_cases.py, e(route) <= min(4 e_ref + 1e-7, 1e-4), on clouds whose graphs are DECIDABLE.

DGCNN rebuilds its kNN graph in feature space in every layer.  At a near tie between the 20th and the 21st nearest row the float32
and the float64 oracle take different neighbours, and e_ref then measures another network, not rounding - the reason the family
was left out of f64_cases.FAMILIES.  Here every case is a seed on which no query of any of the four graphs (xyz, x1, x2, x3) sits
near a tie (``MARGIN``), in every masked cloud and for every weight variant the case is run with.  Every correct implementation
then makes the float64 oracle's choices, and the ordinary bar applies.  ``find_seed`` (``python tests/dgcnn_f64_cases.py --search``)
walks consecutive seeds and returns the first such one on which, besides, the float32 oracle's graphs equal the float64 ones;
``SEEDS`` holds what it found.  Tests never search.

Masked rows.  The masked points of a cloud are identical copies of the centre in every layer, so which of them a list names
changes no value.  Neighbour sets are therefore compared after mapping every masked row to the cloud's first masked row
(``canonical_sets``), and the margin treats the copies as ONE row of multiplicity M (the kernels' compact layout): where the copies
straddle the 20 | 21 boundary, what decides the set is the gap between the centre and the kept rows next to it on either side,
and both must meet ``MARGIN`` (stricter than exempting the exact tie alone: a kept row that changes sides with the centre enters
or leaves the list).

Poses.  The stress shape also runs with base weights under scale 0.5, scale 2.0 and the translation 0.5 (1,1,1) / sqrt 3 (``POSE``,
f64_cases.POSES: the ends of the pose sweeps' grids), masked with the posed cloud's centre.  Each pose has a seed of its own from the
same ``find_seed`` under the same MARGIN and SEARCH_LIMIT; all three were found at 40 points (tries 1, 12 and 14).

Sizes left out: 1024 points and beyond - the N > 1024 L2-gather EdgeConv path among them - stay with the golden and oracle tests of
tests/test_dgcnn_gpu.py.  With thousands of queries per cloud and layer no seed meets the condition.

Importing this module touches no GPU.  Not collected by pytest (no test_ prefix)."""
import sys

import numpy as np

import f64_cases as F
import probes
import weight_variants as V

K = 20
GRAPHS = ("xyz", "x1", "x2", "x3")         # the input of layer 1 .. 4's kNN (models/dgcnn.py: self included)
# A query q with exact squared distances d20 <= d21 to its 20th and 21st nearest rows is decidable when
#     (d21 - d20) / (2 (|q|^2 + d21)) >= MARGIN.
# From csrc/iq_dgcnn_knn.h: knn_kernel hands a query to the exact re-ranking when its float32 gap is below
# kNearTie * 2 (|q|^2 + d) + 7.7e-6 * d with kNearTie = 1e-5, i.e. at most (1e-5 + 7.7e-6 / 2) = 1.4e-5 of the scale 2 (|q|^2 + d);
# its float32 selection compares in 32-ulp buckets, 32 * 2^-24 = 1.9e-6 of a value that is at most that scale.  3e-5 lies outside
# both bands with 1.4e-5 to spare for the rounding of the float32 features and distances themselves (about 1e-6 of the scale), so
# the refined ranking AND the float32-only ranking (tuning key 5 = 20) must both give the float64 graph.
MARGIN = 3e-5
SEARCH_LIMIT = 1000
# the weights the mutation tests round to 16 significant bits (f64_cases.trunc16): conv5 (three bf16 terms, csrc/iq_linear.hip) and
# the heads; the EdgeConv layers of 64 / 128 inputs.  (Those run on the fp32 MFMA in edge_fused_kernel today - `cin == 64 || cin ==
# 128` in csrc/iq_dgcnn.hip puts the kNN DISTANCES of these layers on the bf16 pipe, not the P / Q product - so truncating them shows
# that the bar would see a 16-bit product there, were one introduced.)
HEAD_LAYERS = ["conv5.0.weight", "linear1.weight", "linear2.weight", "linear3.weight"]
EDGE_LAYERS = ["conv2.0.weight", "conv3.0.weight", "conv4.0.weight"]

# name -> ((n, r, nc, b), wide): the smallest sizes at which the DGCNN kernels change path
SHAPES = {
    "stress": ((40, 8, 2, 8), False),      # every variant of f64_cases.VARIANTS
    "min": ((21, 8, 1, 4), False),         # 21 rows: the coalitions have fewer than 21 distinct rows
    "edge": ((33, 8, 1, 3), False),        # one row over a 32-row pad
    "n64": ((64, 8, 1, 4), False),         # both sides of two pads / one wave of queries
    "n65": ((65, 8, 1, 3), False),
    "walk": ((40, 8, 1, 8), False),        # nc * 8 <= b: the layer-1 graph comes from the neighbour-list walk
    "wide": ((40, 128, 2, 8), True),       # the wide entry
    "n128": ((128, 8, 1, 2), False),       # four pads; the largest size at which the condition is still cheap to meet
    # the stress shape under the ends of the pose sweeps' grids (``POSE``; f64_cases.POSES), masked with the posed cloud's centre
    "scale_lo": ((40, 8, 2, 8), False),
    "scale_hi": ((40, 8, 2, 8), False),
    "shift": ((40, 8, 2, 8), False),
}
POSE = {"scale_lo": "s0.5", "scale_hi": "s2.0", "shift": "t+"}
SEARCH_START = {name: 9000 + 1000 * i for i, name in enumerate(SHAPES)}
# The stress size has a seed per variant.  Under the margin above (the centre's copies as one row, gaps on both sides) about one seed
# in twelve qualifies for ONE variant at this size, and the walk from 9000 found none for all five at once within SEARCH_LIMIT
# (with the exact tie of two copies merely exempted it is one in four, which is how a common seed can be found - but then a kept
# row next to the centre may change sides, and the float32-only ranking need not give the float64 graph).  Every variant still runs
# on the stress shape, each on clouds that are decidable for it.
SEARCHES = [("stress", (v,)) for v in F.VARIANTS] + [(name, ("base",)) for name in SHAPES if name != "stress"]
# what ``find_seed(name, variants, SEARCH_START[name])`` returned for every entry of SEARCHES
SEEDS = {
    ("stress", "base"): 9010,        # try 11
    ("stress", "seed1"): 9001,       # try 2
    ("stress", "dead"): 9000,        # try 1
    ("stress", "negshift"): 9002,    # try 3
    ("stress", "varspread"): 9019,   # try 20
    ("min", "base"): 10001,          # try 2
    ("edge", "base"): 11000,         # try 1
    ("n64", "base"): 12005,          # try 6
    ("n65", "base"): 13007,          # try 8
    ("walk", "base"): 14002,         # try 3
    ("wide", "base"): 15029,         # try 30
    ("n128", "base"): 16079,         # try 80
    ("scale_lo", "base"): 17000,     # try 1
    ("scale_hi", "base"): 18011,     # try 12
    ("shift", "base"): 19013,        # try 14
}


def make_case(name, seed):
    (n, r, nc, b), wide = SHAPES[name]
    return F.Case(name, probes.CoalitionCase("dgcnn", n, r, nc, b, seed), wide=wide, pose=POSE.get(name))


def pairs():
    """[(case, variant)]: every variant on the stress size, ``base`` elsewhere."""
    return [(make_case(name, SEEDS[name, v]), v) for name, vs in SEARCHES for v in vs]


def pair_id(p):
    return "%s-%s" % (p[0].id, p[1])


def stress_case():
    return make_case("stress", SEEDS["stress", "base"])


# ---- the two extra coalitions of the centre-multiplicity test -----------------------------------------------------------------

def multiplicity_inputs(case):
    """-> the dict of ``f64_cases.inputs`` (without ``member``) for two coalitions of the case's cloud 0: the first keep mask, counting
    up from 1, that masks 19, 20 or 21 points (around k), and the empty coalition, where every row is the centre.  None if no mask
    of the cloud does."""
    i, s = F.inputs(case), case.spec
    assert not case.wide
    rid, cloud, centre = i["rid"][0], i["clouds"][0], i["centers"][0]
    for keep in range(1, (1 << s.r) - 1):
        kept = ((keep >> rid) & 1).astype(bool)
        if K - 1 <= int((~kept).sum()) <= K + 1:
            break
    else:
        return None
    kept = np.stack([kept, np.zeros(s.n, dtype=bool)])
    masked = np.where(kept[:, :, None], cloud[None], centre[None, None, :]).astype(np.float32)
    return dict(clouds=i["clouds"], centers=i["centers"], rid=i["rid"], cloud_of=np.zeros(2, dtype=np.int32), keep=[keep, 0], kept=kept,
                masked=masked)


# ---- graphs: margins and canonical neighbour sets -------------------------------------------------------------------------------

def graph_margins(x, masked_rows):
    """x (B,N,C) float64, masked_rows (B,N) bool -> (B,N) the margin of every query, the copies of the centre taken as one row of
    multiplicity M (module docstring); inf where no kept row lies on the far side of a boundary."""
    x = np.asarray(x, dtype=np.float64)
    b, n, _ = x.shape
    assert n > K
    out = np.empty((b, n))
    for c in range(b):
        m = masked_rows[c]
        if m.any():
            assert (x[c][m] == x[c][m][0]).all(), "masked rows are not identical copies"
        d = ((x[c][:, None, :] - x[c][None, :, :]) ** 2).sum(-1)                 # exact up to float64 rounding, self included
        qq = (x[c] ** 2).sum(-1)
        order = np.argsort(d, axis=1, kind="stable")
        ds = np.take_along_axis(d, order, axis=1)
        plain = (ds[:, K] - ds[:, K - 1]) / (2 * (qq + ds[:, K]))
        straddle = m[order[:, K - 1]] & m[order[:, K]]
        if straddle.any():
            dc = d[:, np.flatnonzero(m)[0]][:, None]                               # the centre's distance
            dk = np.where(m[None, :], np.nan, d)                                   # kept rows only
            with np.errstate(invalid="ignore"):
                lo = np.where(dk <= dc, dk, -np.inf).max(axis=1)                   # the kept row just ahead of the centre
                hi = np.where(dk > dc, dk, np.inf).min(axis=1)                     # and just behind it
            dc = dc[:, 0]
            ahead = np.where(np.isfinite(lo), (dc - lo) / (2 * (qq + dc)), np.inf)
            with np.errstate(invalid="ignore"):
                behind = np.where(np.isfinite(hi), (hi - dc) / (2 * (qq + hi)), np.inf)
            plain = np.where(straddle, np.minimum(ahead, behind), plain)
        out[c] = plain
    return out


def canonical_sets(idx, masked_rows):
    """idx (B,N,k) neighbour rows, masked_rows (B,N) bool -> (B,N,N) bool: the neighbour SET of every query after mapping every
    masked row to the cloud's first masked row."""
    idx = np.asarray(idx).astype(np.int64)
    b, n, _ = idx.shape
    assert idx.min() >= 0 and idx.max() < n
    out = np.zeros((b, n, n), dtype=bool)
    for c in range(b):
        canon = np.arange(n)
        if masked_rows[c].any():
            canon[masked_rows[c]] = np.flatnonzero(masked_rows[c])[0]
        out[c][np.arange(n)[:, None], canon[idx[c]]] = True
    return out


def graph_features(masked, aux, dtype):
    """The four graph inputs of an oracle run as (B,N,C) torch tensors of ``dtype``."""
    import torch
    xyz = torch.as_tensor(np.asarray(masked)).to(getattr(torch, dtype))
    return [xyz] + [aux[k].permute(0, 2, 1).contiguous() for k in GRAPHS[1:]]


def _graphs(masked, aux, dtype, masked_rows):
    """f64_cases._choices for DGCNN: [(name, canonical sets)] of the four graphs the oracle run of ``dtype`` made."""
    from oracle import ref_cpu as O
    return [(name + " kNN", canonical_sets(O.knn(x.permute(0, 2, 1).contiguous(), K).numpy(), masked_rows))
            for name, x in zip(GRAPHS, graph_features(masked, aux, dtype))]


# ---- the two oracle runs ------------------------------------------------------------------------------------------------------

def run_inputs(inp, sd, only_f64=False):
    """-> dict: f64 (and f32: the logits, float64 arrays (b,10)), e_ref, bar, choices {"float32" / "float64": [(name, sets)]},
    margins {graph: (B,N)} of the float64 run, x32 {graph: (B,N,C) float32 array, the float32 oracle's graph inputs}."""
    masked, rows = inp["masked"], ~inp["kept"]
    out = {"choices": {}}
    for dt in ("float64",) if only_f64 else ("float64", "float32"):
        logits, aux = V.oracle_forward("dgcnn", sd, masked, dt, return_aux=True)
        out["f" + dt[-2:]] = logits.double().numpy()
        out["choices"][dt] = _graphs(masked, aux, dt, rows)
        feats = graph_features(masked, aux, dt)
        if dt == "float64":
            out["margins"] = {g: graph_margins(x.numpy(), rows) for g, x in zip(GRAPHS, feats)}
        else:
            out["x32"] = {g: x.numpy() for g, x in zip(GRAPHS, feats)}
    if not only_f64:
        out["e_ref"] = F.rel_err(out["f32"], out["f64"])
        out["bar"] = F.bar(out["e_ref"])
    return out


def min_margin(run):
    """-> (the smallest margin of the run, its graph)."""
    return min((float(m.min()), g) for g, m in run["margins"].items())


def decidable(run):
    return min_margin(run)[0] >= MARGIN


_RUNS = {}


def oracle_run(case, variant, multiplicity=False):
    """``run_inputs`` on the case's coalitions (``multiplicity``: on ``multiplicity_inputs``), computed once."""
    key = (case, variant, multiplicity)
    if key not in _RUNS:
        inp = multiplicity_inputs(case) if multiplicity else F.inputs(case)
        _RUNS[key] = run_inputs(inp, V.variant("dgcnn", variant))
    return _RUNS[key]


# ---- seeds --------------------------------------------------------------------------------------------------------------------

def qualifies(case, variants):
    """Decidable in float64 and the float32 graphs equal to the float64 ones, for every variant; the stress case with ``base`` weights also for
    the two coalitions of the centre-multiplicity test."""
    todo = [(F.inputs(case), v) for v in variants]
    if case.name == "stress" and "base" in variants:
        extra = multiplicity_inputs(case)
        if extra is None:
            return False
        todo.append((extra, "base"))
    for inp, v in todo:                          # the cheap rejection first: one float64 run
        if not decidable(run_inputs(inp, V.variant("dgcnn", v), only_f64=True)):
            return False
    return all(not F.choice_mismatches(run_inputs(inp, V.variant("dgcnn", v))) for inp, v in todo)


def find_seed(name, variants, start, limit=SEARCH_LIMIT):
    """The first seed in [start, start + limit) on which case ``name`` qualifies for every variant of ``variants``, or None."""
    for seed in range(start, start + limit):
        case = make_case(name, seed)
        ok = qualifies(case, variants)
        F._INPUTS.pop(case, None)
        if ok:
            return seed
    return None


if __name__ == "__main__":
    if sys.argv[1:] != ["--search"]:
        sys.exit("usage: python tests/dgcnn_f64_cases.py --search")
    for name_, variants_ in SEARCHES:
        seed_ = find_seed(name_, variants_, SEARCH_START[name_])
        print("(%r, %r): %s,   # try %s" % (name_, variants_[0], seed_, "-" if seed_ is None else seed_ - SEARCH_START[name_] + 1), flush=True)
