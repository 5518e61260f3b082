"""GPU: DGCNN's graphs and every route of its logits against a float64 run of the CPU oracle, on clouds with decidable graphs
(tests/dgcnn_f64_cases.py; tests/test_dgcnn_f64_cpu.py shows what this relies on).

Graphs first, so that a failure is tied to a layer before the logits are looked at: ``hip_ops.knn`` on xyz and on the float32
oracle's x1, x2, x3 must give the float64 oracle's canonical neighbour sets for EVERY query - no mismatch allowance, these cases have
no near ties - under the default (three-term bf16 distances, near ties re-ranked exactly), under the twins "knn_fp32_rank" (5 = 20,
float32 ranking only) and "knn_fp32_mfma" (5 = 22, distances on the fp32 MFMA).  ``hip_ops.knn`` takes multiples of 32 rows: other sizes are padded with rows far
from every point, which are nobody's neighbours and whose own lists are not looked at.

Logits: with e(x) = max |x - float64| / max |float64| over the logits of a case, every route must satisfy
    e(route) <= min(FACTOR e(float32 CPU oracle) + 1e-7, 1e-4),   FACTOR = 4   (f64_cases.bar).
Routes, one printed row each (name, e_hip, e_ref, e_hip / e_ref, bar): the dense ``forward_points`` on the uploaded host-masked
clouds; the coalition entry (``coalition_logits`` with ``cloud_of``; case ``wide``: ``coalition_logits_wide`` at R = 128); both again
under twins 7 / 8 (EdgeConv as GEMM + gather), 12 (no neighbour-list walk), 20, 22 (above) and 57 (dense layers on the fp32 MFMA).
iq_mask_coalitions (_wide) with the host's float32 centre reproduces the host-masked clouds bit for bit, so the CPU test and
this one see the same bytes.

Measured e_hip / e_ref, smallest .. largest over the twelve (case, variant) pairs, from one run of this file on an MI355X (gfx950; the
26 ids in 4 s; e_ref there 4.8e-07 .. 1.9e-06).  Nothing was above the bar, the worst route used 0.81 of it, so FACTOR is 4 on every
route and no kernel was changed.
  graphs     144 comparisons (12 pairs x 4 graphs x keys 0, 20, 22): no query with another neighbour set
  forward_points, alone and under each of 5 = 7, 8, 12, 20, 22, 57 (the same figures to three digits)      0.90 (wide) .. 2.91 (edge)
  coalition entry, alone and under each of 5 = 7, 8, 12, 20, 22, 57 (the same figures to three digits)     1.12 (n65) .. 3.32 (min)
             (the twins agree because they are built to: 7 / 8 / 12 are bit-for-bit relations of tests/test_dgcnn_gpu.py, 20 / 22 give
             the same graphs on these clouds, and 57 changes nothing in DGCNN, whose heads run on the fp32 MFMA whatever the key)
  centre multiplicity (M = 20 and the empty coalition), either entry, alone and under 5 = 12, 20           1.41
  weights with 16 significant bits on the device (last test): every route 39 x e_ref, i.e. 9.5 x the bar
Since then the stress shape also runs under scale 0.5, scale 2.0 and a translation of 0.5 (cases ``scale_lo``, ``scale_hi``, ``shift``:
fifteen pairs, 32 ids, 180 graph comparisons, still no query with another neighbour set).  On these three, e_ref 9.0e-07 .. 1.1e-06:
forward_points and its twins 2.11 (shift) .. 2.90 (scale_hi), the coalition entry and its twins 2.01 (shift) .. 2.60 (scale_hi);
the worst used 0.70 of the bar.
Checked once by hand: a library in which the centre row weighs M + 1 in the mean pool (dg_compact_kernel's row_w) fails the coalition
entry of all twelve pairs and the multiplicity test, at 1e-3 to 3e-3 of max |logit| - below the 1e-2 that DGCNN is held to elsewhere.
"""
import argparse

import numpy as np
import pytest
import torch

import dgcnn_f64_cases as D
import f64_cases as F
import probes
import weight_variants as V
from interpret_quality_amd import hip_ops, synth
from interpret_quality_amd.tuning import tuned

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TWINS = ("edge_gemm_l2", "edge_gemm_lds", "knn_compact", "knn_fp32_rank", "knn_fp32_mfma", "dense_fp32")
KNN_KEYS = (None, "knn_fp32_rank", "knn_fp32_mfma")      # the default, float32 ranking only, distances on the fp32 MFMA
# per route, where it is not f64_cases.FACTOR: (factor, measured ratio, reason) - none so far
FACTORS = {}


def upload(inp, wide, r):
    """The host inputs on the device; the mask kernel with the host's centre writes the host's bytes."""
    up = lambda k: torch.from_numpy(np.ascontiguousarray(inp[k])).to(DEV)
    d = {k: up(k) for k in ("clouds", "centers", "rid", "cloud_of", "masked")}
    d["keep"] = hip_ops.wide_masks_to_tensor(inp["keep"], DEV) if wide else hip_ops.masks_to_tensor(inp["keep"], DEV)
    for c in range(inp["clouds"].shape[0]):
        sel = np.flatnonzero(inp["cloud_of"] == c)
        if not len(sel):
            continue
        keep = d["keep"][torch.from_numpy(sel).to(DEV)].contiguous()
        args = (d["clouds"][c].contiguous(), d["rid"][c].contiguous(), keep, d["centers"][c].contiguous())
        got = hip_ops.mask_coalitions_wide(*args, r) if wide else hip_ops.mask_coalitions(*args)
        assert probes.bitwise_equal(got.cpu().numpy(), inp["masked"][sel]), c
    return d


_DEVICE = {}


def device_inputs(case, multiplicity=False):
    key = (case, multiplicity)
    if key not in _DEVICE:
        _DEVICE[key] = upload(D.multiplicity_inputs(case) if multiplicity else F.inputs(case), case.wide, case.spec.r)
    return _DEVICE[key]


def routes(case, model, d, twins=TWINS):
    """[(name, callable -> logits tensor)]"""
    dense = lambda: model.forward_points(d["masked"])
    if case.wide:
        entry = "coalition_logits_wide"
        coal = lambda: model.coalition_logits_wide(d["clouds"], d["centers"], d["rid"], d["keep"], d["cloud_of"], num_regions=case.spec.r)
    else:
        entry = "coalition_logits"
        coal = lambda: model.coalition_logits(d["clouds"], d["centers"], d["rid"], d["keep"], d["cloud_of"], num_regions=case.spec.r)
    out = [("forward_points", dense), (entry, coal)]
    for key in twins:
        out.append(("forward_points, %s" % key, lambda key=key: tuned(key, dense)))
        out.append(("%s, %s" % (entry, key), lambda key=key: tuned(key, coal)))
    return out


def measure(tag, rows, run):
    """Runs every route, prints its row, -> [(name, e_hip, bar)]."""
    out = []
    for name, fn in rows:
        got = fn().cpu().numpy()
        assert got.shape == run["f64"].shape and np.isfinite(got).all(), (tag, name)
        e_hip, e_ref = F.rel_err(got, run["f64"]), run["e_ref"]
        bar = F.bar(e_ref, FACTORS.get(name, (F.FACTOR,))[0])
        print("%-44s %-34s e_hip %.3g  e_ref %.3g  e_hip / e_ref %.2f  (bar %.3g)" % (tag, name, e_hip, e_ref, e_hip / e_ref, bar))
        out.append((name, e_hip, bar))
    return out


def above(got):
    return ["%s: e_hip %.3g above %.3g" % r for r in got if not r[1] <= r[2]]


def hip_graph(x, far):
    """hip_ops.knn on (B,N,C) float32 rows, padded to a multiple of 32 rows with rows at ``far`` in every channel -> (B,N,20)."""
    b, n, c = x.shape
    pad = -n % 32
    xp = np.concatenate([x, np.full((b, pad, c), far, dtype=np.float32)], axis=1) if pad else x
    got = hip_ops.knn(torch.from_numpy(np.ascontiguousarray(xp)).to(DEV), D.K).cpu().numpy()[:, :n]
    assert got.min() >= 0 and got.max() < n, "a padding row was taken as a neighbour"
    return got


@pytest.mark.parametrize("pair", D.pairs(), ids=D.pair_id)
def test_graphs_are_the_float64_graphs(pair):
    case, variant = pair
    run = D.oracle_run(case, variant)
    assert D.decidable(run) and F.choice_mismatches(run) == []
    rows = ~F.inputs(case)["kept"]
    wrong = []
    for (name, want), g in zip(run["choices"]["float64"], D.GRAPHS):
        x = run["x32"][g]
        far = np.float32(100.0 * max(1.0, float(np.abs(x).max())))
        for key in KNN_KEYS:
            got = D.canonical_sets(tuned(key, lambda: hip_graph(x, far)), rows)
            bad = int((got != want).any(axis=-1).sum())
            print("%-44s %-8s %-13s queries with another neighbour set: %d of %d" % (D.pair_id(pair), name, key, bad, rows.size))
            if bad:
                wrong.append((name, key, bad))
    assert not wrong, wrong


@pytest.mark.parametrize("pair", D.pairs(), ids=D.pair_id)
def test_every_route_is_within_the_float64_bar(pair):
    case, variant = pair
    model, _ = probes.coalition_model("dgcnn", DEV, variant)
    run = D.oracle_run(case, variant)
    assert D.decidable(run) and F.choice_mismatches(run) == []
    got = measure(D.pair_id(pair), routes(case, model, device_inputs(case)), run)
    assert len(got) == 2 + 2 * len(TWINS)
    assert not above(got), above(got)


def test_centre_multiplicity_around_k_and_the_empty_coalition():
    """Two coalitions of the stress case's cloud 0: M = 19, 20 or 21 masked points - around k, where the cut behind the weighted
    centre row changes from "ranks among the 20" to "everything behind the centre falls out" - and the empty coalition, where
    every row is the centre.  The coalition entry (one centre row of weight M in the mean pool) and the dense forward on the
    materialised clouds, both against float64: a multiplicity off by one moves the mean pool by 1 / N."""
    case = D.stress_case()
    model, _ = probes.coalition_model("dgcnn", DEV, "base")
    run = D.oracle_run(case, "base", multiplicity=True)
    assert D.decidable(run) and F.choice_mismatches(run) == []
    masked = (~D.multiplicity_inputs(case)["kept"]).sum(axis=1)
    got = measure("multiplicity M = %d, %d" % tuple(masked), routes(case, model, device_inputs(case, True), twins=("knn_compact", "knn_fp32_rank")), run)
    assert not above(got), above(got)


def test_a_lost_bf16_term_is_above_the_bar_on_the_device():
    """The HIP model loaded with weights of 16 significant bits (conv5 and the heads, and the EdgeConv layers 2 - 4), against float64
    of the TRUE weights: every route is above the bar on the stress case, as the float32 oracle is in tests/test_dgcnn_f64_cpu.py -
    which also shows that these weights leave the graphs as they were.  So the bar resolves, on the device, the loss it is meant to
    catch."""
    from interpret_quality_amd.dgcnn import DGCNN_cls
    case = D.stress_case()
    run = D.oracle_run(case, "base")
    model = DGCNN_cls(argparse.Namespace(dataset="modelnet10", k=20))
    model.load_state_dict(synth.to_torch(F.trunc16(V.variant("dgcnn", "base"), D.HEAD_LAYERS + D.EDGE_LAYERS)))
    got = measure("trunc16 " + case.id, routes(case, model.to(DEV).eval(), device_inputs(case)), run)
    assert len(got) == 2 + 2 * len(TWINS)
    for name, e_hip, bar in got:
        print("%-34s %.2f x the bar" % (name, e_hip / bar))
        assert e_hip > bar, (name, e_hip, bar)
