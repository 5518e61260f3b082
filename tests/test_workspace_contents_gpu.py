"""GPU: no result depends on what lent memory held before the call, and no call writes outside the size it asked for.

Every workspace, scratch and output tensor of a route is handed out by tests/guarded_alloc.py: exactly the size asked, between
two guard zones, filled beforehand with ZERO, ONES (0xFF) or STALE (the bytes a donor call - the same route on the same shape,
other clouds, masks and weights - left in its buffers, allocation by allocation; the module docstring there says why these three
fills and no other).  Each route runs ``plain`` first - as the suite runs it today, unpatched - then under ZERO, ONES and STALE.
Asserted per route: logits (PointNet: also trans_feat and crt) bit for bit the ``plain`` result under every fill, every guard
intact, and the engine asked for a workspace exactly once per call.

The reference chain ends outside the code under test: ``plain`` on exactly these cases is what tests/test_f64_families_gpu.py,
tests/test_dgcnn_f64_gpu.py and tests/test_stress_weights_gpu.py hold to the float64 oracle.  tests/test_guarded_alloc_cpu.py shows
on CPU tensors that the same classes detect a missing clear and a 1-byte overrun; only the device differs here.

(a) engines   one id per (family, case): the cases of f64_cases.cases for pointnet2 / pointconv / gcnn and of dgcnn_f64_cases
              (base weights) for dgcnn, every route of test_f64_families_gpu.routes / test_dgcnn_f64_gpu.routes (dense forward,
              coalition entry narrow or wide, PointConv's walk forced on and off, every twin); four PointNet cases (narrow with
              repeated masks, narrow with two clouds, wide, prefix from permutations) with trans_feat / crt returned.
(b) PointConv's kept tables: iq_pointconv_tables_bytes names all of what a second call on the same tensors re-uses, nothing else.
(c) ``OPS``: one small seeded call per allocating hip_ops wrapper (tests/test_guarded_alloc_cpu.py holds the table complete).
(d) the benchmark's own sequence at toy size through final_common.shap_sampling_all_regions_batch.

Measured, one run of this file on an MI355X (gfx950): the 128 ids in 7.5 s (the slowest, PointConv's stress case with its 14
routes, 1.2 s); 457 routes, 1369 (route x fill) runs (three per route; the driver under ONES only).  Every fill gave the plain
bits on every route and no guard was touched, so no kernel, no ``*_bytes`` formula and no wrapper was changed; ``hip_ops.knn``'s
Python size formula holds in exactly its bytes at C = 3 and C = 64.
Checked once by hand that the file bites where include/iq.h's promise is easiest to break: a library built without the sa1
``hipMemsetAsync`` of csrc/iq_pointnet2.hip (the output the grouped kernel merges into with an atomic max) passes ZERO and ONES
- 0xFFFFFFFF is -1 and loses every signed max - and fails ``stress-pointnet2 forward_points`` under STALE.
"""
import argparse

import numpy as np
import pytest
import torch

import dgcnn_f64_cases as D
import f64_cases as F
import guarded_alloc as G
import probes
import smooth_cases
import test_dgcnn_f64_gpu as Tdg
import test_f64_families_gpu as Tfam
import test_fuzz_gpu as Z
from interpret_quality_amd import _lib, final_common, hip_ops, synth
from interpret_quality_amd.tuning import tuned

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
DONOR_SEED = 50000          # added to a case's seed: other clouds, region ids, masks and cloud_of on the same shape
DONOR_VARIANT = "seed1"
RUNS = {"routes": 0, "fills": 0}     # (route x fill) runs of this process, printed by the last test


def tensors(out):
    """The tensors of a result (tensor, tuple / list, dict; None and ints dropped) as a list."""
    if isinstance(out, torch.Tensor):
        return [out]
    if isinstance(out, dict):
        return [t for k in sorted(out) for t in tensors(out[k])]
    if isinstance(out, (tuple, list)):
        return [t for o in out for t in tensors(o)]
    return []


def same_bits(a, b):
    """Two lists of tensors: as many, and every pair of one dtype, one shape and the same bytes (NaN payloads included)."""
    if len(a) != len(b):
        return False
    for x, y in zip(a, b):
        if x.dtype != y.dtype or x.shape != y.shape:
            return False
        if x.numel() and not torch.equal(x.contiguous().reshape(-1).view(torch.uint8), y.contiguous().reshape(-1).view(torch.uint8)):
            return False
    return True


def under_fills(tag, fn, donor_fn, workspaces=None, rows_differ=False):
    """``fn`` plain, then under ZERO, ONES and STALE (donor: ``donor_fn`` under ZERO) -> the plain tensors."""
    plain = tensors(fn())
    torch.cuda.synchronize()
    RUNS["routes"] += 1

    def one(fill_name, fill):
        with G.guarded(fill) as rec:
            got = tensors(fn())
        RUNS["fills"] += 1
        assert len(rec) >= 1 and all(g.buf.is_cuda for g in rec), (tag, fill_name)
        if workspaces is not None:      # one workspace per call, and the logits in a guarded tensor of their own
            assert len(rec.workspaces) == workspaces and len(rec) > workspaces, (tag, fill_name, len(rec.workspaces), len(rec))
        assert same_bits(got, plain), "%s: the result under %s is not the plain result" % (tag, fill_name)
        return rec

    one("ZERO", G.ZERO)
    one("ONES", G.ONES)
    with G.guarded(G.ZERO) as donor:
        other = tensors(donor_fn())
    if rows_differ:         # the stale bytes really are another call's
        assert bool((other[0] != plain[0]).any(dim=1).all()), "%s: a row of the donor's logits equals the recipient's" % tag
    rec = one("STALE", G.STALE(donor))
    assert rec.sizes() == donor.sizes()
    return plain


def test_the_guards_are_compared_on_the_device():
    """What tests/test_guarded_alloc_cpu.py shows on CPU tensors, once on the device: a byte written behind a body (inside the
    buffer that holds the guard) is reported with its side and offset, and a STALE body holds the donor's bytes."""
    g = G.Guarded(1000, G.ONES, DEV)
    g.check()
    torch.as_strided(g.body, (1001,), (1,))[-1] = 7
    with pytest.raises(G.GuardError, match="tail guard .* changed at offset 0 of"):
        g.check()
    donor = G.Guarded(1000, G.ZERO, DEV)
    donor.body.copy_(torch.arange(1000, device=DEV).to(torch.uint8))
    assert torch.equal(G.Guarded(1000, G.STALE(donor), DEV).body, donor.body)


# ---- (a) engines ------------------------------------------------------------------------------------------------------------------

def donor_of(case):
    return case._replace(spec=case.spec._replace(seed=case.spec.seed + DONOR_SEED))


FAMILY_CASES = [(f, c) for f in F.FAMILIES for c in F.cases(f)]
DGCNN_CASES = [c for c, v in D.pairs() if v == "base"]


@pytest.mark.parametrize("family,case", FAMILY_CASES, ids=["%s" % c.id for _, c in FAMILY_CASES])
def test_family_routes_under_hostile_workspaces(family, case):
    model, _ = probes.coalition_model(family, DEV, "base")
    other, _ = probes.coalition_model(family, DEV, DONOR_VARIANT)
    rows = Tfam.routes(family, case, model)
    donors = Tfam.routes(family, donor_of(case), other)
    assert [n for n, _ in rows] == [n for n, _ in donors] and len(rows) == 2 + 2 * len(Tfam.TWINS[family]) + 2 * (family == "pointconv")
    for (name, fn), (_, dfn) in zip(rows, donors):
        under_fills("%s %s" % (case.id, name), fn, dfn, workspaces=1, rows_differ=True)


@pytest.mark.parametrize("case", DGCNN_CASES, ids=[c.id for c in DGCNN_CASES])
def test_dgcnn_routes_under_hostile_workspaces(case):
    model, _ = probes.coalition_model("dgcnn", DEV, "base")
    other, _ = probes.coalition_model("dgcnn", DEV, DONOR_VARIANT)
    rows = Tdg.routes(case, model, Tdg.device_inputs(case))
    donors = Tdg.routes(donor_of(case), other, Tdg.device_inputs(donor_of(case)))
    assert len(rows) == 2 + 2 * len(Tdg.TWINS)
    for (name, fn), (_, dfn) in zip(rows, donors):
        under_fills("%s %s" % (case.id, name), fn, dfn, workspaces=1, rows_differ=True)


PN = lambda n, r, nc, b, k: probes.CoalitionCase("pointnet", n, r, nc, b, 8100 + k)
POINTNET_CASES = [F.Case("narrow-repeats", PN(200, 8, 1, 40, 0)), F.Case("narrow", PN(1024, 32, 2, 70, 1)),
                  F.Case("wide", PN(300, 128, 2, 24, 2), wide=True), F.Case("prefix", PN(200, 65, 1, 3, 3), wide=True)]
PN_DISTINCT = 13            # the first case's 40 masks are these many, repeated


def pointnet_routes(case, model):
    """[(name, callable -> (logits, trans_feat[, crt]))] at the engine, so that the optional outputs are guarded tensors too."""
    i, s = F.inputs(case), case.spec
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    clouds, centers, rid, cloud_of = up(i["clouds"]), up(i["centers"]), up(i["rid"]), up(i["cloud_of"])
    eng = model.engine()
    if case.name == "prefix":
        rng = np.random.default_rng(s.seed)
        orders = hip_ops.as_i32(np.stack([rng.permutation(s.r) for _ in range(s.b)]), DEV)
        return [("prefix_logits_wide", lambda: eng.prefix_logits_wide(clouds, centers, rid, orders, None, num_regions=s.r, return_trans_feat=True))]
    if case.wide:
        keep = hip_ops.wide_masks_to_tensor(i["keep"], DEV)
        return [("coalition_logits_wide", lambda: eng.coalition_logits_wide(clouds, centers, rid, keep, cloud_of, num_regions=s.r,
                                                                            return_trans_feat=True))]
    masks = [i["keep"][j % PN_DISTINCT] for j in range(s.b)] if case.name == "narrow-repeats" else i["keep"]
    keep = hip_ops.masks_to_tensor(masks, DEV)
    run = lambda: eng.coalition_logits(clouds, centers, rid, keep, cloud_of, num_regions=s.r, return_trans_feat=True, return_crt=True)
    return [("coalition_logits", run), ("coalition_logits, chain_no_dedup", lambda: tuned("chain_no_dedup", run))]


@pytest.mark.parametrize("case", POINTNET_CASES, ids=[c.id for c in POINTNET_CASES])
def test_pointnet_routes_under_hostile_workspaces(case):
    model, _ = probes.coalition_model("pointnet", DEV, "base")
    other, _ = probes.coalition_model("pointnet", DEV, DONOR_VARIANT)
    rows, donors = pointnet_routes(case, model), pointnet_routes(donor_of(case), other)
    for (name, fn), (_, dfn) in zip(rows, donors):
        plain = under_fills("%s %s" % (case.id, name), fn, dfn, workspaces=1, rows_differ=True)
        assert len(plain) == (2 if case.wide else 3) and bool(torch.isfinite(plain[0]).all())


# ---- (b) PointConv's kept tables -----------------------------------------------------------------------------------------------

def test_pointconv_keeps_its_tables_in_the_first_tables_bytes_and_nowhere_else():
    """One persistent Guarded workspace of exactly the size asked.  After the first call the tables are built (state 3).  Every
    byte BEHIND iq_pointconv_tables_bytes(nc, N) overwritten with 0xFF: the second call on the same tensors re-uses the tables and
    gives the same bits.  Then the head overwritten too and the engine's memory of the tables cleared: the same bits again."""
    case = F.stress_base("pointconv")
    model, _ = probes.coalition_model("pointconv", DEV, "base")
    d, s = Tfam.device_inputs(case), case.spec
    eng = model.engine()
    clouds, centers = d["clouds"].clone(), d["centers"].clone()
    call = lambda: eng.coalition_logits(clouds, centers, d["rid"], d["keep"], d["cloud_of"])
    plain = call().clone()
    head = int(_lib.load().iq_pointconv_tables_bytes(s.nc, s.n))
    need = int(eng.coalition_bytes(s.b, s.nc, s.n))
    assert 0 < head < need
    g = G.Guarded(need, G.ONES, DEV, "PointConv's persistent workspace")
    eng._ws = None
    eng.workspace_replaced()
    eng._ws = g.body
    try:
        first = call()
        assert eng._ws is g.body and eng._tab["state"] == 3
        key = eng._tab["key"]
        g.check()
        g.body[head:].fill_(0xFF)
        second = call()
        assert eng._ws is g.body and eng._tab["state"] == 3 and eng._tab["key"] == key
        g.check()
        g.body.fill_(0xFF)
        eng._tab = {}
        third = call()
        assert eng._tab["state"] == 3
        g.check()
    finally:
        eng._ws = None
        eng.workspace_replaced()
    assert same_bits([first], [plain]) and same_bits([second], [plain]) and same_bits([third], [plain])


# ---- (c) hip_ops wrappers ----------------------------------------------------------------------------------------------------------

def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _rng(*key):
    return np.random.default_rng(list(key))


def _cloud(rng, n):
    return up(rng.standard_normal((n, 3)).astype(np.float32))


def _orders(rng, s, r):
    return hip_ops.as_i32(np.stack([rng.permutation(r) for _ in range(s)]), DEV)


def _pack(member):
    """(M,R) bool -> (M,W) uint64 keep rows."""
    m, r = member.shape
    bit = np.left_shift(np.uint64(1), (np.arange(r) & 63).astype(np.uint64))
    return np.stack([np.where(member[:, 64 * w:64 * w + 64], bit[64 * w:64 * w + 64], np.uint64(0)).sum(axis=1, dtype=np.uint64)
                     for w in range((r + 63) // 64)], axis=1)


def _sampled_rows(rng, r, units, paired, narrow):
    """Keep rows of ``units`` sampled coalitions (neither empty nor full), each followed by its complement when ``paired``."""
    member = rng.random((units, r)) < 0.5
    member[:, 0], member[:, 1] = True, False
    if paired:
        member = np.stack([member, ~member], axis=1).reshape(2 * units, r)
    words = _pack(member)
    return hip_ops.masks_to_tensor(words[:, 0], DEV) if narrow else hip_ops.wide_masks_to_tensor(words, DEV)


def _game(rng, m, g=3):
    return (up(rng.standard_normal((g, m)).astype(np.float32)), up(rng.standard_normal(g)), up(rng.standard_normal(g)))


def _mt_state(seed):
    return hip_ops.mt_state_to_device(DEV, np.random.RandomState(seed).get_state())


def op_mask(kind, n):
    def build(seed):
        rng = _rng(seed, n)
        cloud, rid8, rid128, center = _cloud(rng, n), hip_ops.as_i32(rng.integers(0, 8, n), DEV), hip_ops.as_i32(rng.integers(0, 128, n), DEV), _cloud(rng, 1)[0]
        if kind == "mask_shapley":
            orders = _orders(rng, 3, 8)
            return lambda: hip_ops.mask_shapley(cloud, rid8, orders, center)
        if kind == "mask_interaction":
            pairs = hip_ops.as_i32(np.array([[0, 1], [5, 2], [7, 3]]), DEV)
            ctx = hip_ops.masks_to_tensor(rng.integers(0, 256, 3), DEV)
            return lambda: hip_ops.mask_interaction(cloud, rid8, pairs, ctx, center, 8)
        if kind == "mask_coalitions":
            keep = hip_ops.masks_to_tensor(rng.integers(0, 256, 5), DEV)
            return lambda: [hip_ops.mask_coalitions(cloud, rid8, keep, center, channel_first=cf) for cf in (False, True)]
        keep = hip_ops.wide_masks_to_tensor(_pack(rng.random((5, 128)) < 0.5), DEV)
        return lambda: [hip_ops.mask_coalitions_wide(cloud, rid128, keep, center, 128, channel_first=cf) for cf in (False, True)]
    return build


def op_knn(c):
    def build(seed):
        x = up(_rng(seed, c).standard_normal((2, 96, c)).astype(np.float32))
        return lambda: hip_ops.knn(x, 20)
    return build


def op_reward(classes):
    def build(seed):
        logits = up(_rng(seed).standard_normal((37, 10)).astype(np.float32))
        if classes:
            return lambda: [hip_ops.reward_classes(logits, None, m) for m in (True, False)]
        return lambda: [hip_ops.reward(logits, 3, m) for m in (True, False)]
    return build


def op_shapley(kind, r):
    def build(seed):
        rng = _rng(seed, r)
        s = 6
        orders = _orders(rng, s, r)
        if kind in ("shapley_accum", "shapley_accum_wide"):
            v = up(rng.standard_normal(s * (r + 1)).astype(np.float32))
            return lambda: getattr(hip_ops, kind)(v, orders, snap_counts=[2, s])
        v = up(rng.standard_normal((3, s * (r + 1))).astype(np.float32))
        return lambda: getattr(hip_ops, kind)(v, orders, snap_counts=[2, s])
    return build


def op_keep_masks(kind):
    def build(seed):
        rng = _rng(seed)
        if kind == "prefix_keep_masks":
            o = _orders(rng, 5, 8)
            return lambda: hip_ops.prefix_keep_masks(o)
        if kind == "prefix_keep_masks_wide":
            o = _orders(rng, 5, 130)
            return lambda: hip_ops.prefix_keep_masks_wide(o)
        r = 8 if kind == "context_keep_masks" else 130
        pairs = np.array([[0, 1], [5, 2], [7, 3]])
        ctx = np.stack([np.stack([rng.choice([x for x in range(r) if x not in pr], size=4, replace=False) for _ in range(2)]) for pr in pairs])
        p, c = hip_ops.as_i32(pairs, DEV), hip_ops.as_i32(ctx, DEV)
        if kind == "context_keep_masks":
            return lambda: hip_ops.context_keep_masks(p, c)
        return lambda: hip_ops.context_keep_masks_wide(p, c, r)
    return build


def op_enum(seed):
    return lambda: [hip_ops.enum_keep_masks(3 + seed, 100, 9, DEV), hip_ops.enum_keep_masks(0, 16, 4, DEV, players=[6, 1, 3, 0], base=1 << 5)]


def op_exact(kind, n):
    def build(seed):
        v = up(_rng(seed, n).standard_normal(1 << n).astype(np.float32))
        return lambda: getattr(hip_ops, kind)(v)
    return build


def op_kshap_masks(wide, paired):
    def build(seed):
        r = 130 if wide else 8
        rng = _rng(seed, r)
        orders, sizes = _orders(rng, 7, r), hip_ops.as_i32(rng.integers(1, r, 7), DEV)
        return lambda: (hip_ops.kshap_keep_masks_wide if wide else hip_ops.kshap_keep_masks)(orders, sizes, paired)
    return build


def op_kshap(kind, r, paired, narrow):
    def build(seed):
        rng = _rng(seed, r)
        keep = _sampled_rows(rng, r, 40, paired, narrow)
        v, v0, delta = _game(rng, keep.shape[0])
        if kind == "kshap_accum":
            return lambda: hip_ops.kshap_accum(keep, v, v0, r)
        if kind == "kshap_moment_wide":
            return lambda: hip_ops.kshap_moment_wide(keep, v, v0, r)
        if kind == "kshap_pairs":
            return lambda: hip_ops.kshap_pairs(keep, v, v0, delta, r)
        if kind == "kshap_pairs_se":
            return lambda: hip_ops.kshap_pairs_se(keep, v, v0, delta, r, paired=paired)
        return lambda: hip_ops.kshap_moment_se(keep, v, v0, r, paired=paired)
    return build


def op_kshap_solve(seed):
    rng = _rng(seed)
    z = rng.standard_normal((40, 8))
    a, b, delta = up(z.T @ z + np.eye(8)), up(rng.standard_normal((3, 8))), up(rng.standard_normal(3))
    return lambda: hip_ops.kshap_solve(a, b, delta)


def op_kshap_analytic(seed):
    rng = _rng(seed)
    b, wsum, delta = up(rng.standard_normal((3, 130))), up(np.array([80.0])), up(rng.standard_normal(3))
    return lambda: hip_ops.kshap_phi_analytic(b, wsum, delta)


def op_draw(r, paired):
    return lambda seed: (lambda: hip_ops.kshap_draw_counter(11 + seed, 2, 5, 33, r, paired=paired, device=DEV))


def op_sample(wide):
    def build(seed):
        state = _mt_state(seed)

        def run():
            hip_ops._sample_ws.pop(DEV, None)       # the per-device cache: the workspace is allocated under the guard
            st = state.clone()
            try:
                if wide:
                    return [hip_ops.sample_permutations_wide(st, 50, 130), st]
                return [hip_ops.sample_permutations(st, 1000, 32), st]        # a call the many-workgroup kernels draw
            finally:
                hip_ops._sample_ws.pop(DEV, None)   # no later call may keep a view of a guarded buffer
        return run
    return build


def op_region_assign(wide):
    def build(seed):
        n, r = (300, 130) if wide else (203, 8)
        rng = _rng(seed, n)
        cloud, idx = _cloud(rng, n), hip_ops.as_i32(rng.choice(n, r, replace=False), DEV)
        return lambda: (hip_ops.region_assign_wide if wide else hip_ops.region_assign)(cloud, idx)
    return build


def op_smooth(wide):
    def build(seed):
        c = smooth_cases.cloud("tiny")
        pts = c.pts + (0.01 * _rng(seed).standard_normal(c.pts.shape)).astype(np.float32) * (seed != 0)
        cloud, rid = up(pts.astype(np.float32)), hip_ops.as_i32(c.rid, DEV)
        fn = hip_ops.smoothness_enum_wide if wide else hip_ops.smoothness_enum
        return lambda: fn(cloud, rid, c.num_regions, "linearity", "inc", epochs=smooth_cases.EPOCHS)
    return build


def op_linear(m, cin, cout, act, bf3):
    def build(seed):
        rng = _rng(seed, m)
        layer = hip_ops.PackedLinear(rng.standard_normal((cout, cin)).astype(np.float32), rng.standard_normal(cout).astype(np.float32), DEV, bf3=bf3)
        x = up(rng.standard_normal((m, cin)).astype(np.float32))
        return lambda: hip_ops.linear(x, layer, act)
    return build


def op_geom(kind, shape):
    def build(seed):
        rng = _rng(seed, *[int(1000 * x) for x in shape])
        if kind == "knn_point":
            b, n, s = shape
            xyz, q = up(Z._cloud(rng, b, n)), up(Z._cloud(rng, b, s))
            return lambda: hip_ops.knn_point(xyz, q, min(n, 2))
        if kind in ("density", "pointconv_inverse_density"):
            b, n, bw = shape
            x = up(Z._ball(rng, b, n, 0.5))
            return lambda: getattr(hip_ops, kind)(x, bw)
        if kind == "sort_neighbours":
            b, s, c, k = shape
            n = 50
            keys, q = up(rng.standard_normal((b, n, c)).astype(np.float32)), up(rng.standard_normal((b, s, c)).astype(np.float32))
            idx = hip_ops.as_i32(rng.integers(0, n, size=(b, s, k)), DEV)
            return lambda: hip_ops.sort_neighbours(q, keys, idx.clone())
        if kind == "fps":
            b, n, s = shape
            x = up(Z._cloud(rng, b, n))
            return lambda: hip_ops.fps(x, s)
        if kind == "ball_query":
            b, n, s, k = shape
            xyz = Z._ball(rng, b, n, 1.0)
            q = xyz[:, rng.integers(0, n, size=s)].copy()
            xyz, q = up(xyz), up(q)
            return lambda: hip_ops.ball_query(xyz, q, 0.5, k)
        c, b, n, s, k = shape
        pts, xyz, ctr = (up(rng.standard_normal(sh).astype(np.float32)) for sh in ((b, n, c), (b, n, 3), (b, s, 3)))
        idx2, idx3, eidx = (up(rng.integers(0, n, size=sh)) for sh in ((b, s), (b, s, k), (b, n, k)))
        if kind == "index_points":
            return lambda: [hip_ops.index_points(pts, idx2), hip_ops.index_points(pts, idx3)]
        if kind == "group_points":
            return lambda: [hip_ops.group_points(xyz, pts, ctr, idx3), hip_ops.group_points(xyz, None, None, idx3)]
        return lambda: [hip_ops.edgeconv_gather(pts, eidx, channel_first=False)]
    return build


def op_check_index_range(seed):
    t = hip_ops.as_i32(_rng(seed).integers(0, 9, 1000), DEV)
    return lambda: hip_ops.check_index_range(t, 0, 9, "t")


def op_pointnet_debug(kind):
    def build(seed):
        keep = hip_ops.masks_to_tensor(_rng(seed).integers(0, 16, 90), DEV)
        return lambda: getattr(hip_ops, kind)(keep, None, num_regions=8)
    return build


def _ops():
    """[(id, the hip_ops wrapper the call exercises, seed -> callable)]"""
    out = [("knn-C%d" % c, "knn", op_knn(c)) for c in (3, 64)]
    out += [("%s-N%d" % (k, n), k, op_mask(k, n)) for k in ("mask_shapley", "mask_interaction", "mask_coalitions", "mask_coalitions_wide")
            for n in (200, 203)]
    out += [("reward", "reward", op_reward(False)), ("reward_classes", "reward_classes", op_reward(True))]
    out += [("shapley_accum-R8", "shapley_accum", op_shapley("shapley_accum", 8)),
            ("shapley_accum_wide-R65", "shapley_accum_wide", op_shapley("shapley_accum_wide", 65))]
    out += [("%s-R%d" % (k, r), k, op_shapley(k, r)) for k in ("shapley_accum_games", "shapley_sq_accum_games") for r in (8, 65)]
    out += [("interaction_reduce", "interaction_reduce",
             lambda seed: (lambda v=up(_rng(seed).standard_normal(4 * 33).astype(np.float32)): hip_ops.interaction_reduce(v)))]
    out += [(k, k, op_keep_masks(k)) for k in ("prefix_keep_masks", "prefix_keep_masks_wide", "context_keep_masks", "context_keep_masks_wide")]
    out += [("enum_keep_masks", "enum_keep_masks", op_enum)]
    out += [("%s-n%d" % (k, n), k, op_exact(k, n)) for k in ("exact_shapley", "exact_interactions", "moebius") for n in (1, 3, 8, 13)]
    out += [("kshap_keep_masks%s-%s" % ("_wide" if w else "", "paired" if p else "unpaired"), "kshap_keep_masks" + ("_wide" if w else ""),
             op_kshap_masks(w, p)) for w in (False, True) for p in (True, False)]
    out += [("kshap_accum-%s" % ("paired" if p else "unpaired"), "kshap_accum", op_kshap("kshap_accum", 8, p, True)) for p in (True, False)]
    out += [("kshap_moment_wide-%s" % ("paired" if p else "unpaired"), "kshap_moment_wide", op_kshap("kshap_moment_wide", 130, p, False))
            for p in (True, False)]
    for k in ("kshap_pairs", "kshap_pairs_se", "kshap_moment_se"):
        out += [("%s-%s-%s" % (k, "narrow" if nar else "wide", "paired" if p else "unpaired"), k, op_kshap(k, 8 if nar else 130, p, nar))
                for nar in (True, False) for p in (True, False)]
    out += [("kshap_solve", "kshap_solve", op_kshap_solve), ("kshap_phi_analytic", "kshap_phi_analytic", op_kshap_analytic)]
    out += [("kshap_draw_counter-R%d-%s" % (r, "paired" if p else "unpaired"), "kshap_draw_counter", op_draw(r, p)) for r in (8, 130) for p in (True, False)]
    out += [("sample_permutations", "sample_permutations", op_sample(False)), ("sample_permutations_wide", "sample_permutations_wide", op_sample(True))]
    out += [("region_assign", "region_assign", op_region_assign(False)), ("region_assign_wide", "region_assign_wide", op_region_assign(True))]
    out += [("smoothness_enum", "smoothness_enum", op_smooth(False)), ("smoothness_enum_wide", "smoothness_enum_wide", op_smooth(True))]
    out += [("linear-M%d-%d-%d-act%d" % (m, ci, co, a), "linear", op_linear(m, ci, co, a, bf3))
            for m, ci, co, a, bf3 in ((129, 40, 256, 0, True), (700, 64, 320, 1, True), (300, 256, 40, 0, False))]
    # the first two entries of the fuzz slice's case lists; FPS: the first workgroup case and the first one-wave-per-cloud case
    geom = [("knn_point", [c for c in Z.KNN_CASES[:2]]), ("density", Z.DENSITY_CASES[:2]), ("pointconv_inverse_density", Z.DENSITY_CASES[:2]),
            ("sort_neighbours", Z.SORT_CASES[:2]), ("index_points", Z.GATHER_CASES[:2]), ("group_points", Z.GATHER_CASES[:2]),
            ("edgeconv_gather", Z.GATHER_CASES[:2]), ("fps", [Z.FPS_CASES[0][:3], Z.FPS_CASES[2][:3]]), ("ball_query", Z.BALL_CASES[:2])]
    for k, shapes in geom:
        out += [("%s-%s" % (k, "-".join("%g" % x for x in sh)), k, op_geom(k, tuple(sh))) for sh in shapes]
    out += [("check_index_range", "check_index_range", op_check_index_range)]
    out += [(k, k, op_pointnet_debug(k)) for k in ("pointnet_reps", "pointnet_slots")]
    return out


OPS = _ops()
assert len({o[0] for o in OPS}) == len(OPS)


@pytest.mark.parametrize("name,wrapper,build", OPS, ids=[o[0] for o in OPS])
def test_hip_ops_wrappers_under_hostile_memory(name, wrapper, build):
    assert Z.FPS_CASES[0][0] < 64 <= Z.FPS_CASES[2][0]          # one FPS case on each side of the wave / workgroup threshold
    under_fills(name, build(0), build(1))


# ---- (d) one driver ------------------------------------------------------------------------------------------------------------------

def test_the_benchmark_sequence_at_toy_size_under_ones():
    """PointNet, N = 200, R = 8, 20 permutations through final_common.shap_sampling_all_regions_batch: phi and the logits are the
    plain run's bits when every workspace and every ``torch.empty`` tensor held 0xFF."""
    n, r, s = 200, 8, 20
    model, _ = probes.coalition_model("pointnet", DEV, "base")
    pts, label = synth.make_cloud(0, num_points=n)
    data, lbl = torch.from_numpy(pts).unsqueeze(0).to(DEV), torch.tensor([label]).to(DEV)
    fps = hip_ops.fps(data, r)[0]
    region_id = hip_ops.region_assign(data[0].contiguous(), fps.contiguous()).cpu().numpy().astype(np.int64)
    orders = synth.make_orders(s, r, seed=1)
    args = argparse.Namespace(model="pointnet", softmax_type="modified", num_points=n, num_regions=r, num_samples=s, shapley_batch_size=4,
                              verbose=False)
    run = lambda: final_common.shap_sampling_all_regions_batch(model, data, lbl, region_id, orders, args)
    phi, logits = run()
    with G.guarded(G.ONES) as rec:
        got_phi, got_logits = run()
    RUNS["routes"] += 1
    RUNS["fills"] += 1
    assert len(rec.workspaces) >= 1 and len(rec) > len(rec.workspaces)
    assert same_bits([got_logits], [logits]) and np.array_equal(np.asarray(got_phi).view(np.uint64), np.asarray(phi).view(np.uint64))
    print("routes %d, (route x fill) runs %d in this process" % (RUNS["routes"], RUNS["fills"]))
