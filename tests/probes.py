"""Randomised-shape probes shared by the collected GPU slice (tests/test_fuzz_gpu.py) and the open-ended probe scripts
(tests/fuzz_sizes.py, tests/fuzz_hotpath.py): frozen case records with readable ids, the code that runs a case on the HIP
path, and the checkers that hold the result to a plain reference.

Importing this module touches no GPU (the model and oracle imports are inside the functions), so case lists can be built at
pytest collection time on a CPU-only machine.  Not collected by pytest itself (no test_ prefix)."""
import argparse
import os
import sys
from typing import NamedTuple

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

FAMILIES = ("pointnet", "pointnet2", "pointconv", "dgcnn", "gcnn")
# cloud sizes each family's coalition path accepts (README: PointNet 1-4096, PointNet++ >= 128, PointConv >= 64, DGCNN / GCNN
# >= 21); the upper ends of the random draws keep the CPU oracle affordable
SIZE_LIMITS = {"pointnet": (1, 4096), "pointnet2": (128, 2100), "pointconv": (64, 2100), "dgcnn": (21, 2100), "gcnn": (21, 2100)}
COALITION_RTOL = 1e-4             # of max |logit|, against the dense HIP forward and against the CPU oracle
DGCNN_ORACLE_RTOL = 1e-2          # DGCNN against the float32 oracle: its feature-space kNN cannot be held tighter (README "Parity")


# ---- coalition paths of the five families -------------------------------------------------------------------------------

class CoalitionCase(NamedTuple):
    """One coalition_logits call: `nc` source clouds of `n` points, `r` regions, `b` coalitions; `seed` fixes the clouds,
    region ids, keep masks and cloud_of."""
    family: str
    n: int
    r: int
    nc: int
    b: int
    seed: int

    @property
    def id(self):
        return "%s-N%d-R%d-nc%d-b%d-s%d" % (self.family, self.n, self.r, self.nc, self.b, self.seed)


def random_coalition_case(rng, family):
    """The draw of fuzz_sizes.py: a size just above the family's minimum or anywhere in its range, R in {1,2,8,32,64}, 1-9
    source clouds (more than 8: no pair tables), 2-89 coalitions (8 per source cloud and more: groups from the source lists)."""
    lo, hi = SIZE_LIMITS[family]
    n = int(rng.choice([rng.integers(lo, min(hi, lo + 40)), rng.integers(lo, hi)]))
    r = int(rng.choice([1, 2, 8, 32, 64]))
    nc = int(rng.choice([1, 2, 3, 9]))
    b = int(rng.choice([rng.integers(2, 12), rng.integers(12, 90)]))
    return CoalitionCase(family, n, r, nc, b, int(rng.integers(0, 2 ** 31)))


def coalition_inputs(case):
    """Host inputs of a case: clouds (nc,n,3) f32, region ids (nc,n) i32, keep masks (b Python ints; the first is the full
    coalition and the last the empty one), cloud_of (b,) i32."""
    from interpret_quality_amd import synth
    rng = np.random.default_rng(case.seed)
    # (make_cloud normalises the centred cloud by its radius: one point would be 0 / 0, so N = 1 takes a 2-point cloud's first)
    clouds = np.stack([synth.make_cloud(int(rng.integers(0, 1000)), num_points=max(case.n, 2))[0][:case.n] for _ in range(case.nc)])
    rid = rng.integers(0, case.r, size=(case.nc, case.n)).astype(np.int32)
    full = (1 << case.r) - 1
    keep = [int(x) & full for x in rng.integers(0, 1 << 63, size=case.b)]
    keep[0], keep[-1] = full, 0
    cloud_of = rng.integers(0, case.nc, size=case.b).astype(np.int32)
    return clouds, rid, keep, cloud_of


_MODELS = {}


def coalition_model(family, device, variant=None):
    """(HIP model, state dict) of a family with the synthetic weights of seed 0, built once per process.  ``variant``: a name
    tests/weight_variants.py's ``variant`` knows ("dead", "rescaled12", ...): that state dict instead, cached beside the base."""
    key = family if variant is None else (family, variant)
    if key not in _MODELS:
        from interpret_quality_amd import synth
        from interpret_quality_amd.dgcnn import DGCNN_cls, GCNN_cls
        from interpret_quality_amd.pointconv import PointConvDensityClsSsg
        from interpret_quality_amd.pointnet import PointNetCls
        from interpret_quality_amd.pointnet2 import PointNet2ClsMsg
        cls, sdf = {"pointnet": (PointNetCls, synth.pointnet_state_dict), "pointnet2": (PointNet2ClsMsg, synth.pointnet2_state_dict),
                    "pointconv": (PointConvDensityClsSsg, synth.pointconv_state_dict), "dgcnn": (DGCNN_cls, synth.dgcnn_state_dict),
                    "gcnn": (GCNN_cls, synth.dgcnn_state_dict)}[family]
        if variant is None:
            sd = synth.to_torch(sdf(0))
        else:
            import weight_variants
            sd = synth.to_torch(weight_variants.variant(family, variant))
        m = cls(argparse.Namespace(dataset="modelnet10", k=20) if "cnn" in family else None)
        m.load_state_dict(sd)
        _MODELS[key] = (m.to(device).eval(), sd)
    return _MODELS[key]


def _first(o):
    return o[0] if isinstance(o, tuple) else o


def oracle_logits(family, sd, masked_bn3):
    """The CPU oracle's logits of (B,N,3) clouds (float32)."""
    import torch
    from oracle import ref_cpu as O
    x = masked_bn3.permute(0, 2, 1).contiguous()
    with torch.no_grad():
        if family == "pointnet":
            return _first(O.PointNetOracle(sd)(x)).numpy()
        if family == "pointnet2":
            return _first(O.PointNet2Oracle(sd)(x)).numpy()
        if family == "pointconv":
            return _first(O.PointConvOracle(sd)(x)).numpy()
        return O.dgcnn_forward(sd, x, 20, family == "gcnn").numpy()


def run_coalition_case(case, device, oracle_cap=None, variant=None):
    """-> (coalition logits, dense HIP logits of the materialised masked clouds, oracle logits or None, masked clouds).
    The oracle runs when the case holds at most `oracle_cap` points in all (None: always).  ``variant``: as coalition_model's."""
    import torch
    from interpret_quality_amd import hip_ops
    m, sd = coalition_model(case.family, device, variant)
    clouds_h, rid_h, keep, cloud_of = coalition_inputs(case)
    clouds = torch.from_numpy(clouds_h).to(device)
    centers = clouds.mean(dim=1)
    rid = torch.from_numpy(rid_h).to(device)
    got = m.coalition_logits(clouds, centers, rid, hip_ops.masks_to_tensor(keep, device),
                             torch.from_numpy(cloud_of).to(device), num_regions=case.r).cpu().numpy()
    masked = torch.empty((case.b, case.n, 3), dtype=torch.float32, device=device)
    for c in range(case.nc):
        sel = np.flatnonzero(cloud_of == c)
        if len(sel):
            masked[torch.from_numpy(sel).to(device)] = hip_ops.mask_coalitions(
                clouds[c].contiguous(), rid[c].contiguous(), hip_ops.masks_to_tensor([keep[i] for i in sel], device),
                centers[c].contiguous())
    if case.family == "pointnet":
        dense = _first(m(masked.permute(0, 2, 1).contiguous())).cpu().numpy()
    else:
        dense = m.forward_points(masked).cpu().numpy()
    want = None
    if oracle_cap is None or case.b * case.n <= oracle_cap:
        want = oracle_logits(case.family, sd, masked.cpu())
    return got, dense, want, masked


def rel_max_err(got, ref):
    """max |got - ref| / max |ref| (float64)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-30))


def coalition_problems(family, got, dense, want=None):
    """Why coalition logits `got` are wrong (empty list: they are right): non-finite entries, more than 1e-4 of max |logit|
    off the dense HIP forward, or off the oracle by more than its bar (DGCNN: 1e-2 against the float32 oracle)."""
    out = []
    if not np.isfinite(got).all():
        out.append("non-finite logits")
    e = rel_max_err(got, dense)
    if not e <= COALITION_RTOL:
        out.append("vs dense %.2g" % e)
    if want is not None:
        e = rel_max_err(got, want)
        tol = DGCNN_ORACLE_RTOL if family == "dgcnn" else COALITION_RTOL
        if not e <= tol:
            out.append("vs oracle %.2g" % e)
    return out


# ---- the hot path (PointNet): FPS, region assignment, Shapley sampling, order interactions ----------------------------------

HOT_LOGIT_RTOL = 1e-4
HOT_PHI_RTOL = 2e-3               # of max |phi|: a difference of nearly equal rewards, each within 1e-4 of the logits
HOT_INTERACTION_ATOL = 2e-4       # the reduction of the SAME logits: exp / log differ in the last bits (fuzz_hotpath.py)
REGION_NEAR_TIE_FRACTION = 0.01   # region ids may differ only at near-ties of two centres


class HotpathCase(NamedTuple):
    """One cloud of `n` points, `r` regions, `s` permutations in batches of `bs`, softmax type `sm`; `seed` fixes the
    cloud, the orders and the interaction pairs / contexts."""
    n: int
    r: int
    s: int
    bs: int
    sm: str
    seed: int

    @property
    def id(self):
        return "hot-N%d-R%d-S%d-bs%d-%s-s%d" % (self.n, self.r, self.s, self.bs, self.sm, self.seed)


def random_hotpath_case(rng):
    """The draw of fuzz_hotpath.py: N in 8..4096, R in {1,2,3,8,17,32,64}, 1-3 permutations per batch, both softmax types."""
    n = int(rng.integers(8, 4097))
    r = int(rng.choice([1, 2, 3, 8, 17, 32, 64]))
    bs = int(rng.choice([1, 2, 3]))
    s = bs * int(rng.integers(1, 4))
    sm = str(rng.choice(["modified", "normal"]))
    return HotpathCase(n, r, s, bs, sm, int(rng.integers(0, 2 ** 31)))


_ORACLES = {}


def run_hotpath_case(case, device):
    """-> dict of the case's results: fps / want_fps, region_id / want_rid, (phi, logits) and the oracle's, the interaction
    logits and rewards (HIP and oracle; None when R < 2)."""
    import torch
    from interpret_quality_amd import final_common, hip_ops, interaction, synth
    from oracle import ref_cpu as O
    model, sd = coalition_model("pointnet", device)
    if "pointnet" not in _ORACLES:
        _ORACLES["pointnet"] = O.PointNetOracle(sd)
    om = _ORACLES["pointnet"]
    rng = np.random.default_rng(case.seed)
    pts, label = synth.make_cloud(int(rng.integers(0, 1000)), num_points=case.n)
    data_c = torch.from_numpy(pts).unsqueeze(0)
    data = data_c.to(device)
    lbl = torch.tensor([label], device=device)
    res = {}
    res["fps"] = hip_ops.fps(data, case.r).cpu().numpy()
    want_fps = O.farthest_point_sample(data_c, case.r)
    res["want_fps"] = want_fps.numpy()
    res["region_id"] = hip_ops.region_assign(data[0].contiguous(), torch.from_numpy(res["fps"][0]).to(device)).cpu().numpy()
    want_rid = np.asarray(O.cal_region_id(data_c, want_fps[0]))
    res["want_rid"] = want_rid
    orders = np.stack([rng.permutation(case.r) for _ in range(case.s)]).astype(np.int64)
    args = argparse.Namespace(model="pointnet", softmax_type=case.sm, num_points=case.n, verbose=False, num_regions=case.r,
                              num_samples=case.s, shapley_batch_size=case.bs)
    phi, logits = final_common.shap_sampling_all_regions_batch(model, data, lbl, want_rid, orders, args)
    o_phi, o_logits = O.shap_sampling_all_regions_batch(om, data_c, torch.tensor([label]), want_rid, orders, case.s, case.bs,
                                                        case.r, case.sm)
    res.update(phi=np.asarray(phi), logits=logits.cpu().numpy(), want_phi=np.asarray(o_phi), want_logits=o_logits.numpy())
    res.update(int_logits=None, want_int_logits=None, int_v=None, want_int_v=None)
    if case.r >= 2:
        # loop C on the same cloud: random pairs, contexts of a random order m (final_point_binary_interaction_logits.py:15-70)
        npair, nctx = int(rng.integers(1, 4)), int(rng.integers(1, 5))
        m_order = int(rng.integers(0, case.r - 1))
        pairs = np.stack([rng.choice(case.r, size=2, replace=False) for _ in range(npair)]).astype(np.int64)
        ctxs = np.stack([np.stack([rng.choice([x for x in range(case.r) if x not in pr], size=m_order, replace=False)
                                   for _ in range(nctx)]) for pr in pairs]).astype(np.int64).reshape(npair, nctx, m_order)
        args.interaction_batch_size = int(rng.integers(1, 4))
        res["int_logits"] = interaction.compute_order_interaction_logits(model, data, want_rid, pairs, ctxs, args).cpu().numpy()
        want_i = O.compute_order_interaction_logits(om, data_c, want_rid, pairs, ctxs, args.interaction_batch_size)
        res["want_int_logits"] = want_i.numpy()
        # the reduction ((v0 + v3) - v1) - v2 (final_cal_interactions.py:28-36) on the SAME logits: a difference of nearly equal
        # rewards, each within 2e-6 of the reference's, so an absolute bar, which still catches a wrong row order
        res["int_v"] = np.asarray(interaction.compute_order_interaction(want_i.to(device), lbl, args))
        res["want_int_v"] = np.asarray(O.compute_order_interaction(want_i, torch.tensor([label]), case.sm))
    return res


def hotpath_errors(res):
    """-> (geometry ok, logits error, phi error, interaction error) as fuzz_hotpath.py prints them."""
    geom_ok = np.array_equal(res["fps"], res["want_fps"]) and (res["region_id"] != res["want_rid"]).mean() <= REGION_NEAR_TIE_FRACTION
    e_l = rel_max_err(res["logits"], res["want_logits"])
    e_p = float(np.abs(res["phi"] - res["want_phi"]).max() / max(np.abs(res["want_phi"]).max(), 1e-6))
    e_i = 0.0
    if res["int_logits"] is not None:
        e_i = rel_max_err(res["int_logits"], res["want_int_logits"])
        if np.abs(res["int_v"] - res["want_int_v"]).max() > HOT_INTERACTION_ATOL:
            e_i = max(e_i, 1.0)
    return geom_ok, e_l, e_p, e_i


def hotpath_problems(res):
    geom_ok, e_l, e_p, e_i = hotpath_errors(res)
    out = []
    if not geom_ok:
        out.append("geometry differs")
    if not e_l <= HOT_LOGIT_RTOL:
        out.append("logits %.2g" % e_l)
    if not e_p <= HOT_PHI_RTOL:
        out.append("phi %.2g" % e_p)
    if not e_i <= HOT_LOGIT_RTOL:
        out.append("interaction %.2g" % e_i)
    if not np.isfinite(res["phi"]).all():
        out.append("non-finite phi")
    return out


# ---- index-valued checkers (kNN, sorted neighbour rows, ball query) ------------------------------------------------------

def set_mismatches(got, want, score, tol):
    """Rows whose index sets differ may differ only by candidates whose scores are within `tol` of each other."""
    bad = 0
    for b in range(got.shape[0]):
        for i in range(got.shape[1]):
            sg, sw = set(got[b, i].tolist()), set(want[b, i].tolist())
            assert len(sg) == got.shape[2], "duplicate neighbour in row (%d,%d)" % (b, i)
            if sg != sw:
                dg, dw = np.sort(score[b, i, list(sg - sw)]), np.sort(score[b, i, list(sw - sg)])
                scale = max(1.0, float(np.abs(score[b, i]).max()))
                assert np.allclose(dg, dw, rtol=0, atol=tol * scale), (b, i, dg, dw)
                bad += 1
    return bad


def assert_rows_nearest_first(idx, dist, tol):
    """dist (B,S,N) distances (smaller = nearer): every row of idx non-decreasing up to `tol` of the row's scale."""
    d = np.take_along_axis(dist, idx.astype(np.int64), axis=2)
    scale = np.maximum(1.0, np.abs(dist).max(axis=2, keepdims=True))
    assert (np.diff(d, axis=2) >= -tol * scale).all()


def ball_mismatch(got, want, xyz, new_xyz, radius, oracle):
    """Index-valued: rows may differ only where a point sits within rounding of the sphere."""
    bad = np.nonzero((got != want).any(axis=-1))
    if len(bad[0]) == 0:
        return 0
    d = oracle.square_distance(new_xyz, xyz).numpy()
    r2 = np.float32(radius ** 2)
    for b, s in zip(*bad):
        near = np.abs(d[b, s] - r2) < 4e-7
        assert near.any(), "ball query row (%d,%d) differs without a boundary point" % (b, s)
    return len(bad[0])


def sqdist64(q, p):
    """Exact-ish squared distances in float64: q (B,S,C), p (B,N,C) -> (B,S,N)."""
    q, p = np.asarray(q, dtype=np.float64), np.asarray(p, dtype=np.float64)
    return np.maximum((q * q).sum(-1)[:, :, None] + (p * p).sum(-1)[:, None, :] - 2 * np.einsum("bsc,bnc->bsn", q, p), 0.0)


KNN_TOL = 1e-6                    # of the row's distance scale: the float32 expanded-form distance (test_geom_ops_gpu.py)


def assert_duplicates_lower_index_first(idx, pts, complete=True):
    """pts (B,N,C): among the entries of a row that name coinciding points (or repeat an index), indices come in non-decreasing
    order; with `complete`, a row that holds a copy of a point also holds every lower-indexed copy (kNN: ties go to the lower
    index)."""
    pts = np.asarray(pts)
    for b in range(idx.shape[0]):
        _, group = np.unique(pts[b], axis=0, return_inverse=True)
        group = group.reshape(-1)
        for s in range(idx.shape[1]):
            row = idx[b, s]
            for g in np.unique(group[row]):
                sel = row[group[row] == g]
                assert (np.diff(sel) >= 0).all(), "row (%d,%d): copies of one point out of index order: %s" % (b, s, sel)
                if complete:
                    copies = np.flatnonzero(group == g)
                    assert set(copies[copies <= sel.max()].tolist()) <= set(sel.tolist()), \
                        "row (%d,%d): a lower-indexed copy of point %d is missing" % (b, s, sel.max())


def check_knn(idx, xyz, new_xyz, k):
    """idx (B,S,k) from knn_point(xyz (B,N,3), new_xyz (B,S,3), k): indices in [0, N), no repeats within a row, rows
    nearest first in float64 distance, and the set equal to the float64 top-k except for candidates at a float32 tie."""
    idx = np.asarray(idx).astype(np.int64)
    b, n = np.asarray(xyz).shape[:2]
    assert idx.shape == (b, np.asarray(new_xyz).shape[1], k), idx.shape
    assert idx.min() >= 0 and idx.max() < n, "index outside [0, %d)" % n
    d64 = sqdist64(new_xyz, xyz)
    want = np.argsort(d64, axis=2, kind="stable")[:, :, :k]
    nbad = set_mismatches(idx, want, -d64, KNN_TOL)
    assert_rows_nearest_first(idx, d64, KNN_TOL)
    return nbad


def f32_distance_bound(q, p, c):
    """A bound on the rounding error of a float32 expanded-form distance |p|^2 - 2 q.p + |q|^2 over `c` channels (element-
    wise, float64): gamma_(c+2) times the sum of the magnitudes it adds up."""
    q, p = np.asarray(q, dtype=np.float64), np.asarray(p, dtype=np.float64)
    mag = (q * q).sum(-1)[:, :, None] + (p * p).sum(-1)[:, None, :] + 2 * np.einsum("bsc,bnc->bsn", np.abs(q), np.abs(p))
    return (c + 3) * 2.0 ** -24 * mag


def check_sorted_rows(out, inp, q, keys):
    """out = sort_neighbours(q (B,S,C), keys (B,N,C), inp) (B,S,k): each row a permutation of its input row, non-decreasing
    in float64 distance up to the float32 rounding bound, coinciding points (and repeated indices) in index order."""
    out, inp = np.asarray(out).astype(np.int64), np.asarray(inp).astype(np.int64)
    assert out.shape == inp.shape, (out.shape, inp.shape)
    assert np.array_equal(np.sort(out, axis=2), np.sort(inp, axis=2)), "a row is not a permutation of its input"
    d64 = np.take_along_axis(sqdist64(q, keys), out, axis=2)
    err = np.take_along_axis(f32_distance_bound(q, keys, np.asarray(keys).shape[2]), out, axis=2)
    step = np.diff(d64, axis=2)
    assert (step >= -(err[:, :, 1:] + err[:, :, :-1])).all(), "a row is not nearest first: step %.3g" % step.min()
    assert_duplicates_lower_index_first(out, keys, complete=False)


# ---- value-valued checkers (density, gathers, FPS) --------------------------------------------------------------------

DENSITY_ORACLE_RTOL = 2e-6        # against oracle.compute_density (float32): the documented contract
DENSITY_F64_RTOL = 1e-4           # against the float64 evaluation: float32 expanded-form distances, not a dropped point
DENSITY_FLOOR = 1e-30             # entries below this (underflow) are compared absolutely


def density64(xyz, bandwidth):
    """models/pointconv.py:199-209 in float64 on exact distances."""
    x = np.asarray(xyz, dtype=np.float64)
    out = np.empty(x.shape[:2])
    for i0 in range(0, x.shape[1], 256):                     # 256 rows at a time: (B,256,N,3) doubles
        d = ((x[:, i0:i0 + 256, None, :] - x[:, None, :, :]) ** 2).sum(-1)
        out[:, i0:i0 + 256] = (np.exp(-d / (2.0 * bandwidth * bandwidth)) / (2.5 * bandwidth)).mean(axis=-1)
    return out


def density_problems(got, want32, want64):
    out = []
    got = np.asarray(got, dtype=np.float64)
    for name, want, tol in (("oracle", want32, DENSITY_ORACLE_RTOL), ("float64", want64, DENSITY_F64_RTOL)):
        want = np.asarray(want, dtype=np.float64)
        e = (np.abs(got - want) / np.maximum(np.abs(want), DENSITY_FLOOR)).max()
        if not e <= tol:
            out.append("vs %s %.3g" % (name, e))
    return out


def rel_err(x, ref64):
    """max |x - ref64| over max |ref64|, in float64: the error figure of the float64-anchored tests."""
    return float(np.abs(np.asarray(x, dtype=np.float64) - ref64).max() / np.abs(ref64).max())


def same_tensors(a, b):
    """Two sequences of torch tensors: as many, and each pair torch.equal."""
    import torch
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def bitwise_equal(got, want):
    """Same shape and the same float32 bits everywhere."""
    got, want = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    return got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))
