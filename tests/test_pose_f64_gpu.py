"""GPU: the coalition routes of PointNet++, PointConv, GCNN and PointNet at the ends of the pose sweeps' grids, against a float64 run
of the CPU oracle, and the promise of pose_sweep.sharded_shapley that a cloud's values do not depend on its batch-mates.

Cases (tests/f64_cases.py ``POSED_PAIRS``; tests/test_pose_f64_cpu.py shows what the bar relies on): the stress, smallest, edge and
1024-point clouds of tests/test_f64_families_gpu.py under scale 0.5 and 2.0, the translation 0.5 (1,1,1) / sqrt 3 and rotations by
+-pi/4 about every axis, masked with the centre of the POSED cloud; a ``sweep`` case per family, one cloud under eight poses through
one ``cloud_of`` launch (what pose_sweep.shapley_over_poses launches).  With e(x) = max |x - float64| / max |float64|, every route of
``test_f64_families_gpu.routes`` must satisfy
    e(route) <= min(4 e(float32 CPU oracle) + 1e-7, 1e-4).
One printed row per route: name, e_hip, e_ref, e_hip / e_ref, bar.  iq_mask_coalitions with the host's centre reproduces the
host-masked bytes (``device_inputs``), and the device poses of pose_sweep.py reproduce the host's: scale_pc and translate_pc bit for
bit, rotate_xyz within 3 x 2^-24 x sum |terms| of the float64 product with its own matrix.

PointNet++: which side of sa1's pair-table capacity every posed case is on is asserted from the host count (``f64_cases.pn2_side``):
the 1024-point cloud at scale 0.5 overflows (316 213 rows against 196 800), so its widest scale runs the grouped MLP at 1024 points.

PointNet (the clouds and helpers of tests/test_stress_weights_gpu.py, weights ``seed1`` and ``negshift``, poses s0.5, s2.0, t+, r+):
coalition path and dense forward against float64 at the same bar, the arg-max rows held by value.

PointConv's fused inverse density (pc_density_kernel) is held on its own through iq_pointconv_inverse_density, at the same bar
against a float64 density: behind the DensityNet its error hardly reaches the logits (a kernel with k2 off by 1e-5 relative passes
every logit row here, the worst at 3.2 x e_ref).

Batch independence across the pair-table capacity (``test_a_clouds_logits_do_not_depend_on_its_batch_mate``,
``test_shapley_over_poses_does_not_depend_on_pose_batch``).  Verdict: BIT-IDENTICAL, nothing had to be fixed.  The table-or-fallback
decision of sa1 is taken for the whole launch, so a cloud's route does flip with its batch-mates (N = 256: B from the grouped MLP to
the table; N = 400: A from the table to the grouped MLP; the sweep of eight scales: the identity pose), but both routes give the same
bits - the same arithmetic per pair row, and a maximum does not depend on order (tests/test_pointnet2_gpu.py holds the table
against the dense forward bit for bit at unit scale).  Every |difference| measured: 0.

Measured on an MI355X (gfx950), one run of this file (86 ids in 66 s; the slowest id, the PointNet++ sweep case, 8 s); e_hip / e_ref smallest .. largest, with the case of the
largest.  Nothing above the bar; the worst route used 0.75 of it.
  pointnet2  19 pairs, e_ref 2.1e-07 .. 9.0e-07
             forward_points = coalition entry = 5 = 21 (either entry)        1.05 .. 2.34  (n1024, s0.5: the overflowing one)
             5 = 56 = 5 = 64 (either entry)                                  0.72 .. 3.03  (n1024, s0.5)
             5 = 57 (either entry)                                           0.63 .. 2.62  (stress, s0.5)
  pointconv  23 pairs, e_ref 6.1e-07 .. 1.5e-05 (1.4e-05 .. 1.5e-05 at scale 2.0: ten times the unit-scale figure, as on the CPU)
             forward_points (also 5 = 14, 15, 31), entry under 5 = 14 = walk off     0.74 .. 2.00  (n1024, s0.5)
             coalition entry = 5 = 31 = walk on                                      0.40 .. 2.00  (n1024, s0.5)
             coalition entry, 5 = 15                                                 0.54 .. 2.00  (n1024, s0.5)
             5 = 56: forward_points 0.51 .. 1.70, coalition entry 0.48 .. 1.54 (stress, t+)
             5 = 57: forward_points 0.34 .. 1.89, coalition entry 0.48 .. 2.43 (edge, t+)
             At scale 2.0 every route sits at 0.4 .. 1.0 x e_ref: the error there is the expanded-form distance's, which the
             float32 reference shares.
  gcnn       19 pairs, e_ref 7.1e-07 .. 1.6e-06; every route and twin                0.57 .. 3.09  (n1024, s0.5)
  pointnet   28 rows (2 weights x 4 poses x 2 sizes x 2 paths, less the dead pair's), e_ref 6.2e-07 .. 1.1e-06; coalition path = dense
                                                                                     1.06 .. 2.94  (negshift, s2.0, N = 200)
  inverse density   36 rows (3 sizes x 4 poses x h = 0.1, 0.2, 0.4), e_ref 1.6e-07 .. 4.8e-05   0.84 .. 2.23  (n1024, s0.5, h = 0.4)
             against the float32 oracle 2.6e-07 .. 7.2e-07.  This test found the one defect of the pull request: the kernel kept one
             running float32 sum per lane over N / 2 terms, and where the bandwidth is as wide as the cloud (all terms near 1, the
             float32 reference at 2e-7) that alone cost 1.7e-6 - 4.7 .. 7.9 x e_ref on the 511-point cloud (unposed, s0.5) and
             5.0 x at 1024 points (s0.5), three ids above the bar.  Not d * k2 and not v_exp_f32: a float32 restatement with an exact
             sum gives 2.0e-7, with the kernel's two accumulators 1.5e-6.  The kernel now sums in blocks of 32 terms.
  rotate_xyz on the device: worst error 0.54 / 0.60 of 3 x 2^-24 x sum |terms| (r+ / r-).
"""
import argparse

import numpy as np
import pytest
import torch

import f64_cases as F
import probes
import test_f64_families_gpu as G
import test_stress_weights_gpu as S
import weight_variants as V
from interpret_quality_amd import hip_ops, pose_sweep, synth

pytestmark = pytest.mark.gpu
DEV = G.DEV


# ---- the device poses are the host poses ----------------------------------------------------------------------------------------

def test_device_poses_reproduce_the_host_poses():
    x = F.inputs(F.stress_base("pointnet2"))["clouds"]                       # (2,160,3) unposed
    xd = torch.from_numpy(x).to(DEV)
    for name in ("s0.5", "s2.0", "s1.25", "id"):
        got = pose_sweep.scale_pc(xd, torch.tensor(F.POSES[name][1], dtype=torch.float32, device=DEV))
        assert probes.bitwise_equal(got.cpu().numpy(), F.apply_pose(x, name)), name
    for name in ("t+", "t-"):
        t = F.trans_vector(F.POSES[name][1])
        got = pose_sweep.translate_pc(xd, torch.from_numpy(t).to(DEV))
        assert probes.bitwise_equal(got.cpu().numpy(), F.apply_pose(x, name)), name
    # t+ is what the translation grid makes of its corner (to the rounding of v / |v| * 0.5)
    grid = pose_sweep.generate_trans_vector(pose_sweep.set_grid_args(argparse.Namespace()), DEV).cpu().numpy()
    assert grid.shape == (216, 3) and np.abs(grid[-1] - F.trans_vector(F.POSES["t+"][1])).max() <= 2.0 ** -24
    for name in ("r+", "r-"):
        angles = torch.tensor(F.POSES[name][1], dtype=torch.float32, device=DEV)
        r_dev = pose_sweep.rotate_xyz(torch.eye(3, device=DEV)[None], angles)[0].cpu().numpy().T      # rows e_j . R^T: exact
        assert np.abs(r_dev.astype(np.float64) - F.rotation(F.POSES[name][1])).max() <= 2.0 ** -22    # float32 sines, two 3 x 3 products
        got = pose_sweep.rotate_xyz(xd, angles).cpu().numpy().astype(np.float64)
        x64, r64 = x.astype(np.float64), r_dev.astype(np.float64)
        bound = 3 * 2.0 ** -24 * (np.abs(x64) @ np.abs(r64).T)
        err = np.abs(got - x64 @ r64.T)
        print("rotate_xyz %s: worst error / bound %.3g" % (name, (err / bound).max()))
        assert (err <= bound).all(), name
        assert np.abs(got - F.apply_pose(x, name)).max() <= 2 * bound.max() + 2.0 ** -21              # and so the host's posed cloud


# ---- every route of the grouped families --------------------------------------------------------------------------------------

@pytest.mark.parametrize("pair", F.POSED_PAIRS, ids=F.pair_id)
def test_every_route_is_within_the_float64_bar_under_poses(pair):
    family, case, variant = pair
    model, _ = probes.coalition_model(family, DEV, variant)
    run = F.oracle_run(family, case, variant)
    assert not F.choice_mismatches(run)
    if family == "pointnet2":
        side = F.pn2_side(case)
        assert side != "between"
        assert (side == "overflows") == ((case.name, case.pose) == ("n1024", "s0.5")), (case.id, side)
    got = G.measure(F.pair_id(pair), G.routes(family, case, model), run)
    assert len(got) == 2 + 2 * len(G.TWINS[family]) + (2 if family == "pointconv" else 0)
    if family == "pointconv":
        state = model.engine()._tab.get("state")
        assert state == 3, state
    above = ["%s: e_hip %.3g above %.3g" % r for r in got if not r[1] <= r[2]]
    assert not above, above


# ---- PointConv's fused inverse density, on its own --------------------------------------------------------------------------------

DENSITY_CASES = [(name, pose) for name in ("stress", "edge", "n1024") for pose in (None, "s0.5", "s2.0", "t+")]


@pytest.mark.parametrize("name,pose", DENSITY_CASES, ids=["%s-%s" % (n, p or "unposed") for n, p in DENSITY_CASES])
def test_pointconv_fused_inverse_density_against_float64(name, pose):
    """pc_density_kernel (csrc/iq_pointconv.hip: exp2(d * k2) on the hardware exponential, d in the expanded form) through
    iq_pointconv_inverse_density, on the masked clouds of a PointConv case (100, 511 - the odd tail - and 1024 rows, masked rows
    piled on the centre) at the three bandwidths of the network.  Behind the DensityNet its error hardly shows in the logits, so it
    is held here directly: with e(x) = max_i |x_i - float64_i| / float64_i over the densities, e(1 / kernel) <= 4 e(float32
    oracle) + 1e-7, the bar of the logits, the float64 density from exact differences (probes.density64)."""
    from oracle import ref_cpu as O
    case = next(c for c in F.cases("pointconv") if c.name == name)._replace(pose=pose)
    x = F.inputs(case)["masked"]
    worst = []
    for bw in (0.1, 0.2, 0.4):
        inv = hip_ops.pointconv_inverse_density(torch.from_numpy(x).to(DEV), bw).cpu().numpy().astype(np.float64)
        want32, want64 = O.compute_density(torch.from_numpy(x), bw).numpy().astype(np.float64), probes.density64(x, bw)
        assert inv.shape == want64.shape and np.isfinite(inv).all() and (inv > 0).all() and want64.min() > probes.DENSITY_FLOOR
        e = lambda d: float((np.abs(d - want64) / want64).max())
        e_hip, e_ref = e(1.0 / inv), e(want32)
        print("%-40s h = %.1f  e_hip %.3g  e_ref %.3g  e_hip / e_ref %.2f  (bar %.3g)  against the float32 oracle %.3g" % (
            case.id, bw, e_hip, e_ref, e_hip / e_ref, F.bar(e_ref), float((np.abs(1.0 / inv - want32) / want32).max())))
        assert e_ref >= 1e-8
        if not e_hip <= F.bar(e_ref):
            worst.append("h = %g: e_hip %.3g above %.3g" % (bw, e_hip, F.bar(e_ref)))
    assert not worst, worst


# ---- PointNet -------------------------------------------------------------------------------------------------------------------

PN_POSES = ("s0.5", "s2.0", "t+", "r+")
# ``negshift`` lowers every ReLU bias.  On the halved cloud the trunk keeps live channels (637 of 1024 on the CPU oracle, so the
# arg-max rows are still held by value) but nothing gets through the head: every coalition gives the same logits and all three
# precisions agree exactly (e_hip = e_ref = 0).  The pair runs, and must give exactly those logits, but measures no rounding.
DEAD_PN = {("negshift", "s0.5")}
_PN = {}


def pn_posed(which, pose):
    """tests/test_stress_weights_gpu.py's ``pn_small`` / ``pn_large`` with the cloud under ``pose`` (centre and masked clouds taken
    from the posed cloud by its ``_case``)."""
    if (which, pose) not in _PN:
        c = S.pn_small() if which == "small" else S.pn_large()
        data = torch.from_numpy(F.apply_pose(c["data"].cpu().numpy(), pose)).to(DEV)
        _PN[which, pose] = S._case(data, c["rid"][0].cpu().numpy(), c["keep"], c["nreg"])
    return _PN[which, pose]


@pytest.mark.parametrize("pose", PN_POSES)
@pytest.mark.parametrize("variant", ("seed1", "negshift"))
def test_pointnet_under_poses_against_float64(variant, pose):
    model, _ = probes.coalition_model("pointnet", DEV, variant)
    sd = V.variant("pointnet", variant)
    for which in ("small", "large"):
        c = pn_posed(which, pose)
        logits, crt = model.engine().coalition_logits(c["data"], c["center"], c["rid"], c["keep_t"], None, num_regions=c["nreg"], return_crt=True)
        d_logits, _, d_crt = model(c["masked"].permute(0, 2, 1).contiguous())
        o = {dt: V.oracle_forward("pointnet", sd, c["masked_h"], dt, return_aux=True) for dt in ("float32", "float64")}
        l32, l64 = o["float32"][0].numpy(), o["float64"][0].numpy()
        tag = "%s %s N=%d " % (variant, pose, c["n"])
        spread = float(np.ptp(l64, axis=0).max() / np.abs(l64).max())
        print("%-44s e_ref %.3g  ptp over coalitions %.3g of max |logit|" % (tag, S.rel_err(l32, l64), spread))
        # the bar is live - the logits move over the coalitions and the float32 oracle is not exact - everywhere but on DEAD_PN
        assert (spread > 1e-3 and S.rel_err(l32, l64) >= 1e-8) == ((variant, pose) not in DEAD_PN), (tag, spread)
        S.assert_within_the_oracles_error(tag + "coalition logits", logits.cpu().numpy(), l32, l64)
        S.assert_within_the_oracles_error(tag + "dense logits", d_logits.cpu().numpy(), l32, l64)
        h32, h64 = o["float32"][3]["trunk"].numpy(), o["float64"][3]["trunk"].numpy()
        assert not S.crt_problems(crt.cpu().numpy(), c["kept"], h64, h32, c["n"]), tag
        assert not S.crt_problems(d_crt.cpu().numpy(), c["kept"], h64, h32, c["n"], centre_index=False), tag


# ---- batch independence across the pair-table capacity -----------------------------------------------------------------------------

def pn2_logits(model, i):
    up = lambda k: torch.from_numpy(np.ascontiguousarray(i[k])).to(DEV)
    return model.coalition_logits(up("clouds"), up("centers"), up("rid"), hip_ops.masks_to_tensor(i["keep"], DEV), up("cloud_of"),
                                  num_regions=8)


@pytest.mark.parametrize("n", F.CAPACITY_N)
def test_a_clouds_logits_do_not_depend_on_its_batch_mate(n):
    """Two source clouds, A as drawn and B = 0.15 A (every pair within sa1's widest radius), four coalitions each.  Whether the
    widest scale of sa1 comes from the pair table is decided for the launch (rows summed over its source clouds against
    nclouds x 192 (N + 1), csrc/iq_pointnet2.hip), so a cloud's route depends on its batch-mate: at N = 256 B overflows alone (66 049
    rows against 49 344) and takes the table beside A (69 572 against 98 688); at N = 400 A fits alone (9 523 against 76 992) and
    takes the grouped MLP beside B (B's 160 801 rows alone exceed the joint 153 984).  Its logits must not: alone and in the pair
    they are the same bits, and every arrangement is within the float64 bar."""
    model, _ = probes.coalition_model("pointnet2", DEV, "base")
    inp = {w: F.capacity_inputs(n, w) for w in ("A", "B", "AB")}
    side = {w: F.pn2_side(i) for w, i in inp.items()}
    assert side == {"A": "fits", "B": "overflows", "AB": "fits" if n == 256 else "overflows"}
    run = F.run_masked("pointnet2", "base", inp["AB"]["masked"])
    assert not F.choice_mismatches(run)
    got = {w: pn2_logits(model, i).cpu().numpy() for w, i in inp.items()}
    alone = np.concatenate([got["A"], got["B"]])
    for name, x in (("A and B alone", alone), ("A and B in one launch", got["AB"])):
        e = F.rel_err(x, run["f64"])
        print("N = %d %-22s e_hip %.3g  e_ref %.3g  e_hip / e_ref %.2f  (bar %.3g)" % (n, name, e, run["e_ref"], e / run["e_ref"], run["bar"]))
        assert e <= run["bar"], (name, e, run["bar"])
    diff = np.abs(alone.astype(np.float64) - got["AB"]).max(axis=1) / np.abs(run["f64"]).max()
    print("N = %d alone against paired, per coalition, of max |logit|: %s" % (n, " ".join("%.2g" % d for d in diff)))
    assert probes.bitwise_equal(got["AB"][:4], got["A"]), "cloud A: its logits depend on its batch-mate"
    assert probes.bitwise_equal(got["AB"][4:], got["B"]), "cloud B: its logits depend on its batch-mate"


SWEEP_SCALES = (1.0, 0.5, 0.3, 0.25, 0.2, 0.15, 0.12, 0.1)


def test_shapley_over_poses_does_not_depend_on_pose_batch():
    """PointNet++ on a 400-point cloud under eight scales, identity first: as one batch of eight the launch holds more pair rows than
    eight tables (the small copies hold all 401^2 pairs), alone the identity fits.  pose_batch = 8 against pose_batch = 1."""
    n, r, s = 400, 8, 4
    model, _ = probes.coalition_model("pointnet2", DEV, "base")
    pts, y = synth.make_cloud(3, n)
    poses_h = np.stack([(pts * np.float32(k)).astype(np.float32) for k in SWEEP_SCALES])
    as_inputs = lambda p: dict(clouds=p, centers=p.mean(axis=1, dtype=np.float32))
    assert F.pn2_side(as_inputs(poses_h)) == "overflows" and F.pn2_side(as_inputs(poses_h[:1])) == "fits"
    assert "between" not in [F.pn2_side(as_inputs(poses_h[k:k + 1])) for k in range(len(SWEEP_SCALES))]
    rid = np.random.default_rng(17).integers(0, r, size=n)
    rid[:r] = np.arange(r)
    orders = synth.make_orders(s, r, seed=3)
    args = argparse.Namespace(model="pointnet2", softmax_type="modified", num_points=n, verbose=False, num_regions=r, num_samples=s,
                              shapley_batch_size=s)
    poses, lbl = torch.from_numpy(poses_h).to(DEV), torch.tensor([y]).to(DEV)
    phi8, logits8 = pose_sweep.shapley_over_poses(model, poses, lbl, rid, orders, args, pose_batch=8)
    phi1, logits1 = pose_sweep.shapley_over_poses(model, poses, lbl, rid, orders, args, pose_batch=1)
    assert phi8.shape == (8, r) and logits8.shape == (8, s * (r + 1), 10) and torch.isfinite(logits8).all()
    worst = (logits8.double() - logits1.double()).abs().amax(dim=(1, 2)) / logits1.double().abs().max()
    print("pose_batch 8 against 1, per pose, of max |logit|: %s" % " ".join("%.2g" % w for w in worst.tolist()))
    assert torch.equal(logits8, logits1) and torch.equal(phi8, phi1)


def test_inverse_density_refuses_what_its_lds_image_cannot_hold():
    from interpret_quality_amd import _lib
    with pytest.raises(_lib.IqError, match="N=3073"):
        hip_ops.pointconv_inverse_density(torch.zeros((1, 3073, 3), device=DEV), 0.1)
    with pytest.raises(_lib.IqError, match="bandwidth"):
        hip_ops.pointconv_inverse_density(torch.zeros((1, 64, 3), device=DEV), 0.0)
    got = hip_ops.pointconv_inverse_density(torch.zeros((2, 3072, 3), device=DEV), 0.1)         # every term exp2(0): density 1 / (2.5 h)
    assert torch.equal(got, torch.full((2, 3072), 0.25, device=DEV))
