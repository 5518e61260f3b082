"""GPU: the standard errors of the regression rows' estimates (include/iq.h, "Standard errors") - iq_kshap_pairs_se
and iq_kshap_moment_se_wide against the restatement of their defining formulas (tests/kshap_se_ref.py), and their bits: `out` is
iq_kshap_pairs, `b` is iq_kshap_moment_wide, se is symmetric with a zero diagonal, two calls agree, a game's bits depend neither on
G nor on a neighbour's NaN rewards.

Tolerances, derived, not measured (u = 2^-53).  Pairs, per entry:
    bound = (U / ((U - 1) M^2)) ((U + 16) u sum_u (|P_u| + 2 |B_u| + |G_u|)  +  2 |S1_ij| bound_S1 / U),
the first term the worst case of S2 = sum P + sum B z_i + sum B z_j + sum G z_i z_j in float64 under any summation order (each of
the four sums has at most U terms whose absolute values add up to the bracket; the 16 for the roundings of mu, d, x, the squares,
the assembly and the square root), bound_S1 = M times kshap_pairs_ref.bound, 5h's bound of the first-moment sum.
phi, per region, the same shape:
    bound = (U / ((U - 1) M^2)) ((U + 16) u (2H)^2 sum_u (|e_u| + |f_u|)  +  2 |S1_i| bound_S1 / U),
    bound_S1 = 2H (2 M + R + 32) u sum_m |d_m|      (b_i and the mean of b: sums of at most M terms of |d_m|, R more for the mean).
Every input is held to bound < 1e-6 var at every entry that is checked, on the CPU from the restatement alone: a loose bound
cannot hide a wrong term.  Largest error / bound observed over the 82 shapes: 0.084 (pairs), 0.050 (phi).  That is why the rows' sizes avoid 2, 3, R-3 and R-2 above 16 regions, where x_u(k)^2 for most pairs is
R^4 / 4 times smaller than the unit's largest square and the worst-case bound of a two-unit variance says nothing.

The one statistical test, ``test_bars_are_calibrated_on_a_pointnet_game``: a 10-region value table of PointNet on synthetic cloud
0, 4000 paired rows, pooled z_rms = RMS of (estimate - exact) / se.  The band was measured ONCE with the CPU restatement over the
50 draw seeds 0 .. 49 (size_law_rows(10, 2000, RandomState(seed))), observed min .. max widened by half its width on each side.
It checks the restatement's calibration, not the kernel's (the kernel is held to the restatement by the bounds above).
Pairs, the 50 values:
    0.958 1.176 0.883 0.960 0.861 0.827 0.959 1.084 1.142 0.998 0.926 1.042 0.821 0.923 0.937 0.813 1.135 0.945 0.924 0.958 0.901 1.008 1.172 0.857 0.878
    0.929 0.919 1.005 1.126 1.250 1.050 0.993 0.932 0.890 1.332 1.081 0.933 1.154 1.085 1.110 1.055 0.952 1.084 0.890 1.074 1.096 1.216 1.225 1.071 0.962
    min .. max 0.8128 .. 1.3319, band 0.5533 .. 1.5914 (mean of the 50: 1.010)
phi, the 50 values:
    1.248 1.114 0.718 1.325 1.093 1.275 1.206 1.018 1.198 1.000 0.952 0.589 0.934 0.915 0.881 0.992 0.667 0.612 1.054 0.444 0.776 1.263 0.930 0.727 0.786
    0.913 1.071 1.478 1.081 1.072 0.564 1.095 0.464 0.935 1.436 1.418 1.254 0.957 0.715 0.870 0.827 1.012 0.864 1.164 0.579 1.242 1.013 1.069 0.972 0.832
    min .. max 0.4443 .. 1.4778, band -0.0724 .. 1.9945 (mean of the 50: 0.972; 10 values an estimate against 45: the wider spread)
"""
import argparse

import numpy as np
import pytest
import torch

import kshap_pairs_ref as pairs_ref
import kshap_se_ref as ref
import probes
from interpret_quality_amd import _lib, exact, hip_ops, kernelshap, synth, wide_kernelshap

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
U53 = 2.0 ** -53

REGIONS = [2, 3, 16, 63, 64, 65, 130, 1024]
UNITS = [2, 3, 255, 256, 257]
CASES = [(r, u, p) for r in REGIONS for u in UNITS for p in (True, False)] + [(16, 65537, True), (16, 65537, False)]   # 65 537 units: two tiles a chunk
PAIRS_BAND = (0.5533, 1.5914)
PHI_BAND = (-0.0724, 1.9945)


def sizes_for(r, units, rng):
    """First-row sizes of ``units`` units: 1 and R-1 always, 0 once there are three, the rest uniform over the sizes the module's
    docstring allows (all of 1 .. R-1 up to 16 regions; above, 1, R-1 and those at least R/4 from both ends)."""
    allowed = [s for s in range(1, r) if r <= 16 or s in (1, r - 1) or min(s, r - s) >= r / 4.0]
    sizes = rng.choice(allowed, size=units)
    sizes[0], sizes[1] = 1, r - 1
    if units >= 3:
        sizes[2] = 0
    return sizes


def rows_for(r, units, paired, rng):
    """-> (M,W) uint64: per unit a uniform subset of its size, paired: followed by its complement within the R bits."""
    sizes = sizes_for(r, units, rng)
    order = np.argsort(rng.random_sample((units, r)), axis=1)
    z = np.zeros((units, r), dtype=np.uint8)
    np.put_along_axis(z, order, (np.arange(r)[None] < sizes[:, None]).astype(np.uint8), axis=1)
    if paired:
        z = np.stack([z, 1 - z], axis=1).reshape(2 * units, r)
    padded = np.zeros((len(z), 64 * ((r + 63) // 64)), dtype=np.uint8)
    padded[:, :r] = z
    return np.ascontiguousarray(np.packbits(padded, axis=1, bitorder="little")).view("<u8").astype(np.uint64)


def pairs_bound(keep, v, v0, r, paired):
    """-> (bound (R,R), var (R,R)) of one game by the module's formula, from the restatement's units alone."""
    x, _ = ref.unit_terms(keep, v, v0, r, paired)
    x = x.astype(np.float64)
    p, b, g = x[:, 0] ** 2, x[:, 1] ** 2 - x[:, 0] ** 2, x[:, 2] ** 2 - 2 * x[:, 1] ** 2 + x[:, 0] ** 2
    units, m = len(x), len(v)
    s1, s2 = ref.pairs_moments(keep, v, v0, r, paired)
    bound_s2 = (units + 16) * U53 * float(np.sum(np.abs(p) + 2 * np.abs(b) + np.abs(g)))
    bound_s1 = m * pairs_ref.bound(keep, v, v0, r)
    scale = units / ((units - 1.0) * m * m)
    var = ref.variance(s1, s2, units, m).astype(np.float64)                 # ref.pairs_var, the sums taken once
    np.fill_diagonal(var, 0.0)
    return scale * (bound_s2 + 2 * np.abs(s1.astype(np.float64)) * bound_s1 / units), var


def phi_bound(keep, v, v0, r, paired):
    """-> (bound (R,), var (R,)) of one game by the module's formula."""
    z = ref.first_rows(keep, r, paired)
    _, d = pairs_ref.terms(v, v0, None, len(v))
    big_d = d[0::2] - d[1::2] if paired else d
    s = z.sum(axis=1).astype(np.float64)
    two_h = 2 * float(pairs_ref.harmonic(r))
    e, f = big_d ** 2 * (1 - 2 * s / r), big_d ** 2 * s * s / (r * r)
    units, m = len(z), len(v)
    s1, s2 = ref.phi_moments(keep, v, v0, r, paired)
    bound_s2 = (units + 16) * U53 * two_h ** 2 * float(np.sum(np.abs(e) + np.abs(f)))
    bound_s1 = two_h * (2 * m + r + 32) * U53 * float(np.abs(d).sum())
    scale = units / ((units - 1.0) * m * m)
    return (scale * (bound_s2 + 2 * np.abs(s1.astype(np.float64)) * bound_s1 / units),
            ref.variance(s1, s2, units, m).astype(np.float64))              # ref.phi_var, the sums taken once


def _device(keep, v, v0, delta):
    return (hip_ops.wide_masks_to_tensor(keep, DEV), torch.from_numpy(v).to(DEV), torch.from_numpy(v0).to(DEV), torch.from_numpy(delta).to(DEV))


WORST = {"pairs": 0.0, "phi": 0.0}


@pytest.mark.parametrize("r,units,paired", CASES)
def test_standard_errors_match_the_restatement_and_their_bits_hold(r, units, paired):
    rng = np.random.RandomState(7919 * r + 2 * units + paired)
    keep = rows_for(r, units, paired, rng)
    m = len(keep)
    v = (rng.standard_normal((3, m)) * 3).astype(np.float32)
    v0, delta = rng.standard_normal(3), rng.standard_normal(3)
    kt, vt, v0t, dt = _device(keep, v, v0, delta)
    tag = "R=%d U=%d %s" % (r, units, "paired" if paired else "unpaired")

    out, se = hip_ops.kshap_pairs_se(kt, vt, v0t, dt, r, paired)
    assert out.shape == se.shape == (3, r, r) and se.dtype == torch.float64
    assert torch.equal(out, hip_ops.kshap_pairs(kt, vt, v0t, dt, r)), tag + ": out is not kshap_pairs"
    assert torch.equal(se, se.transpose(1, 2)) and not bool(torch.diagonal(se, dim1=1, dim2=2).any()), tag
    again = hip_ops.kshap_pairs_se(kt, vt, v0t, dt, r, paired)
    assert torch.equal(out, again[0]) and torch.equal(se, again[1]), tag + ": two calls"
    b, var = hip_ops.kshap_moment_se(kt, vt, v0t, r, paired)
    assert b.shape == var.shape == (3, r) and var.dtype == torch.float64
    assert torch.equal(b, hip_ops.kshap_moment_wide(kt, vt, v0t, r)[0]), tag + ": b is not kshap_moment_wide"
    again = hip_ops.kshap_moment_se(kt, vt, v0t, r, paired)
    assert torch.equal(b, again[0]) and torch.equal(var, again[1]), tag + ": two calls"
    for g in range(3):                                              # a game's bits depend neither on G nor on its place
        one = [t[g:g + 1].contiguous() for t in (vt, v0t, dt)]
        o1, s1 = hip_ops.kshap_pairs_se(kt, one[0], one[1], one[2], r, paired)
        b1, v1 = hip_ops.kshap_moment_se(kt, one[0], one[1], r, paired)
        assert torch.equal(o1[0], out[g]) and torch.equal(s1[0], se[g]) and torch.equal(b1[0], b[g]) and torch.equal(v1[0], var[g]), (tag, g)
    poisoned = vt.clone()
    poisoned[1] = float("nan")                                      # the games never meet
    o2, s2 = hip_ops.kshap_pairs_se(kt, poisoned, v0t, dt, r, paired)
    b2, v2 = hip_ops.kshap_moment_se(kt, poisoned, v0t, r, paired)
    for got, clean in ((o2, out), (s2, se), (b2, b), (v2, var)):
        assert torch.equal(got[0], clean[0]) and torch.equal(got[2], clean[2]), tag + ": a game beside NaN rewards"
    assert bool(torch.isnan(s2[1]).any()) and bool(torch.isnan(v2[1]).any())

    upper = np.triu_indices(r, 1)
    bound, want = pairs_bound(keep, v[0], v0[0], r, paired)
    assert np.all(bound[upper] < 1e-6 * want[upper]), tag + ": the pairs bound says too little on this input"
    err = np.abs(se[0].cpu().numpy() ** 2 - want)[upper]
    WORST["pairs"] = max(WORST["pairs"], float((err / bound[upper]).max()))
    print("%s pairs: max error / bound %.3g (bound / var at most %.3g)" % (tag, (err / bound[upper]).max(), (bound[upper] / want[upper]).max()))
    assert np.all(err <= bound[upper]), tag
    bound, want = phi_bound(keep, v[0], v0[0], r, paired)
    assert np.all(bound < 1e-6 * want), tag + ": the phi bound says too little on this input"
    err = np.abs(var[0].cpu().numpy() - want)
    WORST["phi"] = max(WORST["phi"], float((err / bound).max()))
    print("%s phi: max error / bound %.3g (bound / var at most %.3g)" % (tag, (err / bound).max(), (bound / want).max()))
    assert np.all(err <= bound), tag
    print("largest error / bound so far: pairs %.3g, phi %.3g" % (WORST["pairs"], WORST["phi"]))


def test_narrow_rows_and_the_python_entries_agree_with_the_wide_rows():
    rng = np.random.RandomState(5)
    keep = rows_for(16, 300, True, rng)
    v = (rng.standard_normal((2, 600)) * 3).astype(np.float32)
    v0, delta = rng.standard_normal(2), rng.standard_normal(2)
    kt, vt, v0t, dt = _device(keep, v, v0, delta)
    narrow = kt[:, 0].contiguous()
    wide_out = hip_ops.kshap_pairs_se(kt, vt, v0t, dt, 16)
    for a, b in zip(wide_out, hip_ops.kshap_pairs_se(narrow, vt, v0t, dt, 16)):
        assert torch.equal(a, b)
    for a, b in zip(hip_ops.kshap_moment_se(kt, vt, v0t, 16), hip_ops.kshap_moment_se(narrow, vt, v0t, 16)):
        assert torch.equal(a, b)
    inter, se = kernelshap.pairs_se(narrow, vt, v0, v0 + delta, 16)
    assert np.array_equal(inter, wide_out[0].cpu().numpy()) and np.array_equal(se, wide_out[1].cpu().numpy())
    assert np.array_equal(inter, kernelshap.pairs(narrow, vt, v0, v0 + delta, 16))
    one, se1 = wide_kernelshap.pairs_se(kt, vt[0].contiguous(), v0[0], v0[0] + delta[0], 16)
    assert one.shape == se1.shape == (16, 16) and np.array_equal(se1, se[0])
    for ks, rows in ((kernelshap, narrow), (wide_kernelshap, kt)):
        phi, bars = ks.phi_se(rows, vt, v0, v0 + delta, 16)
        assert np.array_equal(phi, ks.estimate(rows, vt, v0, v0 + delta, 16, None, "analytic"))
        assert np.array_equal(bars, np.sqrt(np.maximum(hip_ops.kshap_moment_se(kt, vt, v0t, 16)[1].cpu().numpy(), 0.0)))
    with pytest.raises(_lib.IqError, match="analytic"):
        kernelshap.phi_se(narrow, vt, v0, v0 + delta, 16, gram="sampled")


def test_refusals():
    z = torch.zeros((1,), dtype=torch.float64, device=DEV)
    for m, paired in ((1, False), (2, True), (5, True)):              # one unit; one unit; odd rows in pairs
        keep = torch.ones((m, 1), dtype=torch.int64, device=DEV)
        v = torch.zeros((1, m), dtype=torch.float32, device=DEV)
        with pytest.raises(_lib.IqError):
            hip_ops.kshap_pairs_se(keep, v, z, z, 8, paired)
        with pytest.raises(_lib.IqError):
            hip_ops.kshap_moment_se(keep, v, z, 8, paired)
    keep = torch.ones((4, 1), dtype=torch.int64, device=DEV)
    v = torch.zeros((1, 4), dtype=torch.float32, device=DEV)
    w = torch.ones((4,), dtype=torch.float64, device=DEV)
    with pytest.raises(_lib.IqError, match="weighted"):
        hip_ops.kshap_pairs_se(keep, v, z, z, 8, True, w)
    with pytest.raises(_lib.IqError, match="weighted"):
        hip_ops.kshap_moment_se(keep, v, z, 8, True, w)
    with pytest.raises(_lib.IqError, match="weighted"):
        kernelshap.pairs_se(keep, v, 0.0, 0.0, 8, True, w)
    args = argparse.Namespace(num_regions=8)
    with pytest.raises(_lib.IqError, match="enumerated"):
        kernelshap.game(None, None, None, None, args, samples="all", gram="analytic", se=True)
    with pytest.raises(_lib.IqError, match="analytic"):
        kernelshap.game(None, None, None, None, args, samples=40, gram="sampled", se=True)


def value_table_of_the_pointnet_game():
    """The (1024,) float32 value table of PointNet on synthetic cloud 0 at 10 regions (the device's own FPS)."""
    pts, y = synth.make_cloud(0, 1024)
    data = torch.from_numpy(np.ascontiguousarray(pts))[None].to(DEV)
    fps = hip_ops.fps(data, 10)[0].contiguous()
    rid = hip_ops.region_assign_wide(data[0].contiguous(), fps).cpu().numpy().astype(np.int64)
    args = argparse.Namespace(model="pointnet", softmax_type="modified", num_points=1024, num_regions=10, verbose=False)
    model, _ = probes.coalition_model("pointnet", DEV)
    return exact.value_table(model, data, torch.tensor([y], device=DEV), rid, args)


def test_bars_are_calibrated_on_a_pointnet_game():
    table = value_table_of_the_pointnet_game()
    th = table.cpu().numpy()
    keep = pairs_ref.size_law_rows(10, 2000, np.random.RandomState(0))
    kt = hip_ops.wide_masks_to_tensor(keep, DEV)
    v = table.index_select(0, kt[:, 0]).contiguous()
    inter, se = kernelshap.pairs_se(kt, v, float(th[0]), float(th[-1]), 10)
    upper = np.triu_indices(10, 1)
    z_pairs = float(np.sqrt(np.mean(((inter - pairs_ref.exact_sii(th, 10))[upper] / se[upper]) ** 2)))
    phi, bars = wide_kernelshap.phi_se(kt, v, float(th[0]), float(th[-1]), 10)
    z_phi = float(np.sqrt(np.mean(((phi - hip_ops.exact_shapley(table).cpu().numpy()) / bars) ** 2)))
    print("z_rms: pairs %.4f (band %s), phi %.4f (band %s)" % (z_pairs, PAIRS_BAND, z_phi, PHI_BAND))
    assert PAIRS_BAND[0] <= z_pairs <= PAIRS_BAND[1]
    assert PHI_BAND[0] <= z_phi <= PHI_BAND[1]
