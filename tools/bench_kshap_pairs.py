#!/usr/bin/env python3
"""Times the all-pairs interaction estimator (``hip_ops.kshap_pairs``: SHAP-IQ on the regression rows) and measures
how many rows a usable interaction map needs (not the flagship workload: that is bench.py).

    python tools/bench_kshap_pairs.py [--out profiles/kshap_pairs.json] [--seeds 20] [--runs 5]
    python tools/bench_kshap_pairs.py --se [--out profiles/kshap_pairs_se.json]      the standard errors, see below
    python tools/bench_kshap_pairs.py --control [--out profiles/kshap_pairs_cv.json] the control variates, see below

Part 1 - time.  PointNet, synthetic cloud 0, (R, M) = (32, 33 000), (128, 129 000) and (1024, 1 025 000), G = 1 game (the cloud's
label) and G = 10 (labels 0 .. 9 from the same forwards).  ``--runs`` runs each after a warm-up, wall clock around a synchronised
call, median and the smallest and largest run:
  * the PointNet forwards of the rows (``rewards``);
  * ``hip_ops.kshap_pairs`` - the whole entry: row sizes, Q on the f64 matrix pipe, L, A, the folds and the assembly, with the
    wrapper's allocations and the coefficient table;
  * the eager PyTorch float64 form of Q ALONE, ``(Z * e[:, None]).T @ Z`` per game, in blocks of ``--block`` rows, Z unpacked from
    the same keep words on the device inside the timed region (the kernel starts from the words too) - and, as
    ``eager_product_only``, the same with the unpacked blocks prepared outside the timed region.
The kernel and the eager form are ALTERNATED in one process.  Reported: the kernel's share of forwards + kernel, the ratio eager /
kernel of the medians, whether the difference exceeds the larger spread, and the float64 rate 2 R^2 M G / time of both (the
kernel builds the blocks on and above the diagonal only: its rate is quoted on the full square for comparison, and on the
multiply-adds it performs).

Part 2 - error.  PointNet, synthetic cloud 0, n = 16 regions, ``--seeds`` seeds: RMS over pairs and seeds of
``kernelshap.pairs_from_table`` against the exact index (the mean over the orders of ``hip_ops.exact_interactions`` of the
cloud's value table) at 100 / 300 / 1000 permutations' worth of rows (c (n + 1), paired), beside the RMS of the exact index
itself.  There is no rival estimator at equal evaluations: the number says how many rows a usable map needs.

``--se`` - the same two parts for ``hip_ops.kshap_pairs_se`` (the estimate and the standard error of every entry).  Time:
``kshap_pairs_se``, ``kshap_pairs`` of the same build and the eager float64 form of BOTH products (Q over the rows, the second
moment's product over the units' first rows) alternated in one process; reported are the ratio se / pairs of the medians (the
arithmetic alone says about 1.5: the second product covers half the rows), whether it exceeds 2 beyond the spread, and the
entry's share of forwards + reduction.  Error: at the same seeds and budgets the pooled z_rms = RMS of (estimate - exact) / se over
pairs and seeds, the RMS and the mean of se, and the RMS error they should reproduce.

``--control`` - the control-variate estimators (``kernelshap.pairs_cv``).  Error: the same seeds and budgets for none (``pairs_se``),
shift and regression: RMS error, mean se and pooled z_rms.  Time: ``kernelshap.pairs_cv(control="regression")`` - the whole entry, both
folds: Gram, fit, surrogate, residual SHAP-IQ with its standard error, the host's combination - and ``control="shift"`` against
``hip_ops.kshap_pairs_se`` of the same build on the same rows, R = 16 / 32 / 64 at 1000 (R + 1) rows, G = 1 and 10, alternated in one
process; reported are the ratios of the medians and each entry's share of forwards + reduction.

``--control --sparse`` - the sparse control alone (``control="sparse"``), merged into the file under "sparse".  Error:
the same seeds and budgets for K = 0, the 48 nearest pairs of FPS centres and all 120 pairs, beside shift and regression.  Bars: at
128 and 1024 regions, 1000 (R + 1) counter-drawn rows, default K, the mean se of sparse against shift on the same rows, for listed
and unlisted pairs (no exact index there: the bars are what 5i calibrated).  Time: the entry with both folds and the wrapper against
``kshap_pairs_se``, the shift and the forwards, at R = 64 with the complete list (beside the regression entry) and at 128 and 1024."""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from interpret_quality_amd import exact, hip_ops, kernelshap, synth, wide_kernelshap  # noqa: E402
from interpret_quality_amd.pointnet import PointNetCls  # noqa: E402

SHAPES = ((32, 33000), (128, 129000), (1024, 1025000))
BUDGETS = (100, 300, 1000)      # permutations' worth of evaluations


def _setup(r, dev):
    model = PointNetCls(None)
    model.load_state_dict(synth.to_torch(synth.pointnet_state_dict(0)))
    model = model.to(dev).eval()
    pts, label = synth.make_cloud(0)
    data, lbl = torch.from_numpy(pts).unsqueeze(0).to(dev), torch.tensor([label], device=dev)
    rid = hip_ops.region_assign_wide(data[0].contiguous(), hip_ops.fps(data, r)[0].contiguous()).cpu().numpy().astype(np.int64)
    args = SimpleNamespace(model="pointnet", softmax_type="modified", num_points=1024, num_regions=r, verbose=False)
    return model, data, lbl, rid, args


def _wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, res


def _spread(times):
    return {"median_seconds": float(np.median(times)), "min_seconds": float(min(times)), "max_seconds": float(max(times)),
            "runs": [float(t) for t in times]}


def _unpack(words, r):
    """(B,W) int64-typed keep words -> (B,R) float64 rows z."""
    shifts = torch.arange(64, device=words.device, dtype=torch.int64)
    return ((words[:, :, None] >> shifts) & 1).reshape(words.shape[0], -1)[:, :r].to(torch.float64)


def _eager_q(words, e, r, block, unpacked=None):
    """sum over row blocks of (Z * e_g[:, None]).T @ Z for every game g -> (G,R,R) float64."""
    out = torch.zeros((e.shape[0], r, r), dtype=torch.float64, device=words.device)
    for k, lo in enumerate(range(0, words.shape[0], block)):
        z = unpacked[k] if unpacked is not None else _unpack(words[lo:lo + block], r)
        for g in range(e.shape[0]):
            out[g] += (z * e[g, lo:lo + block, None]).T @ z
    return out


def _unit_g(words, v2, v0, coef, sizes, r):
    """The eager form's per-unit scalar of the second product, G_u = x(2)^2 - 2 x(1)^2 + x(0)^2 of paired rows -> (G,U) float64."""
    mu = torch.stack([coef[:, 0], coef[:, 0] + coef[:, 1], coef[:, 0] + 2 * coef[:, 1] + coef[:, 2]], dim=1)
    mu[1, 2] = 0.0
    d = v2.to(torch.float64) - v0[:, None]
    s = sizes[0::2]
    x = d[:, 0::2, None] * mu[s][None] + d[:, 1::2, None] * mu[r - s].flip(1)[None]
    return x[..., 2] ** 2 - 2 * x[..., 1] ** 2 + x[..., 0] ** 2


def time_shape(r, m, games, runs, block, dev, se=False):
    model, data, lbl, rid, args = _setup(r, dev)
    ks = kernelshap if r <= kernelshap.MAX_REGIONS else wide_kernelshap
    np.random.seed(1)
    keep = kernelshap.draw(r, m, True, dev)[0] if ks is kernelshap else wide_kernelshap.draw_counter(r, m, 1, 0, True, dev)[0]
    classes = None if games == 1 else list(range(games))
    forwards = lambda: ks.rewards(model, data, None if classes else lbl, rid, args, keep, classes=classes)      # noqa: E731
    ks.rewards(model, data, lbl, rid, args, keep[:4096].contiguous())          # warm-up: engine, workspace, code objects
    fwd = []
    for _ in range(runs):
        t, (v, v_full, v_empty) = _wall(forwards)
        fwd.append(t)
    v2, v0, v1 = kernelshap.games(keep, v, v_empty, v_full)
    delta = v1 - v0
    words = keep.reshape(len(keep), -1)
    coef = torch.from_numpy(kernelshap.pair_coefficients(r)).to(dev)
    sizes = _unpack(words, r).sum(dim=1).to(torch.int64) if r <= 128 else torch.cat(
        [_unpack(words[lo:lo + block], r).sum(dim=1).to(torch.int64) for lo in range(0, len(words), block)])
    e = (v2.to(torch.float64) - v0[:, None]) * coef[sizes, 2][None]
    unpacked = None
    if 8 * r * len(words) <= 16 << 30:
        unpacked = [_unpack(words[lo:lo + block], r) for lo in range(0, len(words), block)]
    kernel_call = lambda: hip_ops.kshap_pairs(keep, v2, v0, delta, r)           # noqa: E731
    kernel_call()
    _eager_q(words, e, r, block)
    if se:
        return _time_se(r, games, runs, block, words, e, _unit_g(words, v2, v0, coef, sizes, r), fwd, kernel_call,
                        lambda: hip_ops.kshap_pairs_se(keep, v2, v0, delta, r, True))
    kern, eager, product = [], [], []
    for _ in range(runs):                                                       # alternated in one process
        kern.append(_wall(kernel_call)[0])
        eager.append(_wall(lambda: _eager_q(words, e, r, block))[0])
        if unpacked is not None:
            product.append(_wall(lambda: _eager_q(words, e, r, block, unpacked))[0])
    f, k, q = (float(np.median(x)) for x in (fwd, kern, eager))
    larger = max(max(kern) - min(kern), max(eager) - min(eager))
    nb = (r + 63) // 64
    square = 2.0 * r * r * len(words) * games
    built = 2.0 * (nb * (nb + 1) // 2) * 4096 * len(words) * games
    out = {"num_regions": r, "rows": int(len(words)), "games": games, "pointnet_forwards": _spread(fwd),
           "coalitions_per_s": (len(words) + 2) / f, "kshap_pairs": _spread(kern), "eager_q": _spread(eager),
           "kshap_pairs_share_of_forwards_plus_reduction": k / (f + k), "eager_over_kernel": q / k,
           "larger_spread_seconds": larger, "difference_exceeds_the_larger_spread": bool(abs(q - k) > larger),
           "kernel_ahead_of_eager": bool(k < q),
           "kernel_tflops_on_the_full_square": square / k / 1e12, "kernel_tflops_on_the_blocks_it_builds": built / k / 1e12,
           "eager_tflops": square / q / 1e12, "eager_block_rows": block}
    if product:
        p = float(np.median(product))
        out.update({"eager_product_only": _spread(product), "eager_product_only_over_kernel": p / k,
                    "eager_product_only_tflops": square / p / 1e12})
    return out


def _time_se(r, games, runs, block, words, e, e2, fwd, pairs_call, se_call):
    """The --se rows of ``time_shape``: kshap_pairs_se, kshap_pairs and the eager form of both products, alternated."""
    first = words[0::2].contiguous()
    eager_both = lambda: (_eager_q(words, e, r, block), _eager_q(first, e2, r, block))      # noqa: E731
    se_call()
    eager_both()
    pairs, with_se, eager = [], [], []
    for _ in range(runs):
        pairs.append(_wall(pairs_call)[0])
        with_se.append(_wall(se_call)[0])
        eager.append(_wall(eager_both)[0])
    f, k, s, q = (float(np.median(x)) for x in (fwd, pairs, with_se, eager))
    spread = max(max(pairs) - min(pairs), max(with_se) - min(with_se))
    return {"num_regions": r, "rows": int(len(words)), "units": int(len(first)), "games": games, "pointnet_forwards": _spread(fwd),
            "kshap_pairs": _spread(pairs), "kshap_pairs_se": _spread(with_se), "eager_both_products": _spread(eager),
            "se_over_pairs": s / k, "larger_spread_seconds": spread, "se_costs_more_than_twice_pairs_beyond_the_spread": bool(s - 2 * k > spread),
            "eager_both_over_se": q / s, "kshap_pairs_se_share_of_forwards_plus_reduction": s / (f + s),
            "kshap_pairs_share_of_forwards_plus_reduction": k / (f + k), "eager_block_rows": block}


CONTROL_REGIONS = (16, 32, 64)
SPARSE_REGIONS = (64, 128, 1024)


def time_control(r, games, runs, dev):
    """The --control rows: pairs_cv (regression, shift) and kshap_pairs_se on 1000 (R + 1) paired rows, alternated."""
    model, data, lbl, rid, args = _setup(r, dev)
    m = kernelshap.default_samples(r)
    np.random.seed(1)
    keep = kernelshap.draw(r, m, True, dev)[0]
    classes = None if games == 1 else list(range(games))
    forwards = lambda: kernelshap.rewards(model, data, None if classes else lbl, rid, args, keep, classes=classes)      # noqa: E731
    kernelshap.rewards(model, data, lbl, rid, args, keep[:4096].contiguous())
    fwd = []
    for _ in range(runs):
        t, (v, v_full, v_empty) = _wall(forwards)
        fwd.append(t)
    v2, v0, v1 = kernelshap.games(keep, v, v_empty, v_full)
    calls = {"kshap_pairs_se": lambda: hip_ops.kshap_pairs_se(keep, v2, v0, v1 - v0, r, True),
             "pairs_cv_shift": lambda: kernelshap.pairs_cv(keep, v2, v0, v1, r, True, "shift"),
             "pairs_cv_regression": lambda: kernelshap.pairs_cv(keep, v2, v0, v1, r, True, "regression")}
    times = {name: [] for name in calls}
    for fn in calls.values():
        fn()
    for _ in range(runs):                                                       # alternated in one process
        for name, fn in calls.items():
            times[name].append(_wall(fn)[0])
    f = float(np.median(fwd))
    med = {name: float(np.median(t)) for name, t in times.items()}
    out = {"num_regions": r, "rows": int(len(keep)), "unknowns": kernelshap.pair_features(r), "games": games, "pointnet_forwards": _spread(fwd)}
    for name, t in times.items():
        out[name] = _spread(t)
        out[name + "_share_of_forwards_plus_reduction"] = med[name] / (f + med[name])
    out["regression_over_pairs_se"] = med["pairs_cv_regression"] / med["kshap_pairs_se"]
    out["shift_over_pairs_se"] = med["pairs_cv_shift"] / med["kshap_pairs_se"]
    out["regression_costs_more_than_the_forwards_it_serves"] = bool(med["pairs_cv_regression"] > f)
    return out


def _centres(data, r):
    """(R,3) float64: the FPS centres of the regions ``_setup`` assigns."""
    return data[0].index_select(0, hip_ops.fps(data, r)[0].to(torch.int64)).cpu().numpy().astype(np.float64)


def sparse_table(n, seeds, dev, counts=(0, 48, 120)):
    """``control_table``'s seeds and budgets for the sparse control at K neighbour pairs, beside shift and regression."""
    model, data, lbl, rid, args = _setup(n, dev)
    table = exact.value_table(model, data, lbl, rid, args)
    ends = table[[0, table.numel() - 1]].cpu().numpy()
    pr = hip_ops.all_pairs(n)
    want = hip_ops.exact_interactions(table).cpu().numpy().mean(axis=1)
    most = max(BUDGETS) * (n + 1)
    lists = {"sparse_%d" % k: kernelshap.neighbour_pairs(_centres(data, n), k) for k in counts}
    names = ("shift", "regression") + tuple(lists)
    err2, se1, z2 = ({(c, b): [] for c in names for b in BUDGETS} for _ in range(3))
    for seed in range(seeds):
        np.random.seed(1000 + seed)
        keep, _ = kernelshap.draw(n, most, True, dev)
        for b in BUDGETS:
            rows = keep[:b * (n + 1) // 2 * 2].contiguous()
            v = table.index_select(0, rows).contiguous()
            for c in names:
                how = {"control": "sparse", "pair_list": lists[c]} if c in lists else {"control": c}
                got, se, _ = kernelshap.pairs_cv(rows, v, float(ends[0]), float(ends[1]), n, True, **how)
                got, se = got[pr[:, 0], pr[:, 1]], se[pr[:, 0], pr[:, 1]]
                err2[c, b].append(float(((got - want) ** 2).mean()))
                se1[c, b].append(float(se.mean()))
                z2[c, b].append(float((((got - want) / se) ** 2).mean()))
    return {"model": "pointnet", "cloud": "synthetic_00", "num_regions": n, "pairs": int(len(pr)), "seeds": seeds,
            "exact_index_rms": float(np.sqrt((want ** 2).mean())),
            "budgets": [{"permutations": b, "rows": b * (n + 1) // 2 * 2,
                         **{c: {"rms_error": float(np.sqrt(np.mean(err2[c, b]))), "mean_se": float(np.mean(se1[c, b])),
                                "z_rms": float(np.sqrt(np.mean(z2[c, b])))} for c in names}} for b in BUDGETS]}


def time_sparse(r, runs, dev):
    """The sparse entry (both folds, the wrapper) on 1000 (R + 1) paired rows against kshap_pairs_se, the shift, the forwards and -
    at 64 regions, where the list is the complete one - the regression entry, alternated; and the bars of sparse against shift on
    those rows, for listed and unlisted pairs."""
    model, data, lbl, rid, args = _setup(r, dev)
    ks = kernelshap if r <= kernelshap.MAX_REGIONS else wide_kernelshap
    m = kernelshap.default_samples(r)
    np.random.seed(1)
    keep = kernelshap.draw(r, m, True, dev)[0] if ks is kernelshap else wide_kernelshap.draw_counter(r, m, 1, 0, True, dev)[0]
    k = r * (r - 1) // 2 if r <= kernelshap.MAX_REGIONS else kernelshap.default_control_pairs(r)
    pairs = kernelshap.neighbour_pairs(_centres(data, r), k)
    forwards = lambda: ks.rewards(model, data, lbl, rid, args, keep)      # noqa: E731
    ks.rewards(model, data, lbl, rid, args, keep[:4096].contiguous())
    fwd = []
    for _ in range(runs):
        t, (v, v_full, v_empty) = _wall(forwards)
        fwd.append(t)
    v2, v0, v1 = kernelshap.games(keep, v, v_empty, v_full)
    calls = {"kshap_pairs_se": lambda: hip_ops.kshap_pairs_se(keep, v2, v0, v1 - v0, r, True),
             "pairs_cv_shift": lambda: kernelshap.pairs_cv(keep, v2, v0, v1, r, True, "shift"),
             "pairs_cv_sparse": lambda: kernelshap.pairs_cv(keep, v2, v0, v1, r, True, "sparse", pair_list=pairs)}
    if ks is kernelshap:
        calls["pairs_cv_regression"] = lambda: kernelshap.pairs_cv(keep, v2, v0, v1, r, True, "regression")
    times = {name: [] for name in calls}
    last = {name: fn() for name, fn in calls.items()}
    for _ in range(runs):                                                       # alternated in one process
        for name, fn in calls.items():
            times[name].append(_wall(fn)[0])
    f = float(np.median(fwd))
    med = {name: float(np.median(t)) for name, t in times.items()}
    out = {"num_regions": r, "rows": int(len(keep)), "listed_pairs": int(k), "unknowns": int(r + k), "games": 1,
           "draw": "stream" if ks is kernelshap else "counter", "pointnet_forwards": _spread(fwd)}
    for name, t in times.items():
        out[name] = _spread(t)
        out[name + "_share_of_forwards_plus_reduction"] = med[name] / (f + med[name])
    out["sparse_over_pairs_se"] = med["pairs_cv_sparse"] / med["kshap_pairs_se"]
    out["sparse_costs_more_than_the_forwards_it_serves"] = bool(med["pairs_cv_sparse"] > f)
    if "pairs_cv_regression" in med:
        out["sparse_over_regression"] = med["pairs_cv_sparse"] / med["pairs_cv_regression"]
        out["sparse_is_regression_bit_for_bit"] = bool(np.array_equal(last["pairs_cv_sparse"][0], last["pairs_cv_regression"][0])
                                                       and np.array_equal(last["pairs_cv_sparse"][1], last["pairs_cv_regression"][1]))
    listed = np.zeros((r, r), dtype=bool)
    listed[pairs[:, 0], pairs[:, 1]] = True
    upper = np.triu(np.ones((r, r), dtype=bool), 1)
    host = lambda x: (x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)).reshape(r, r)      # noqa: E731
    se = {name: host(last[name][1]) for name in ("kshap_pairs_se", "pairs_cv_shift", "pairs_cv_sparse")}
    out["mean_se"] = {which: {name: float(x[mask].mean()) for name, x in se.items()}
                      for which, mask in (("all", upper), ("listed", listed), ("unlisted", upper & ~listed)) if mask.any()}
    out["sparse_over_shift_mean_se"] = {which: row["pairs_cv_sparse"] / row["pairs_cv_shift"] for which, row in out["mean_se"].items()}
    out["sparse_beats_shift"] = bool(out["sparse_over_shift_mean_se"]["all"] < 1.0)
    return out


def control_table(n, seeds, dev):
    """``error_table``'s seeds and budgets for none / shift / regression: the error, the bars and their calibration."""
    model, data, lbl, rid, args = _setup(n, dev)
    table = exact.value_table(model, data, lbl, rid, args)
    ends = table[[0, table.numel() - 1]].cpu().numpy()
    pr = hip_ops.all_pairs(n)
    want = hip_ops.exact_interactions(table).cpu().numpy().mean(axis=1)
    most = max(BUDGETS) * (n + 1)
    controls = ("none", "shift", "regression")
    err2, se1, z2 = ({(c, b): [] for c in controls for b in BUDGETS} for _ in range(3))
    for seed in range(seeds):
        np.random.seed(1000 + seed)
        keep, _ = kernelshap.draw(n, most, True, dev)
        for b in BUDGETS:
            rows = keep[:b * (n + 1) // 2 * 2].contiguous()
            v = table.index_select(0, rows).contiguous()
            for c in controls:
                if c == "none":
                    got, se = kernelshap.pairs_se(rows, v, float(ends[0]), float(ends[1]), n)
                else:
                    got, se, _ = kernelshap.pairs_cv(rows, v, float(ends[0]), float(ends[1]), n, True, c)
                got, se = got[pr[:, 0], pr[:, 1]], se[pr[:, 0], pr[:, 1]]
                err2[c, b].append(float(((got - want) ** 2).mean()))
                se1[c, b].append(float(se.mean()))
                z2[c, b].append(float((((got - want) / se) ** 2).mean()))
    return {"model": "pointnet", "cloud": "synthetic_00", "num_regions": n, "pairs": int(len(pr)), "seeds": seeds,
            "exact_index_rms": float(np.sqrt((want ** 2).mean())),
            "budgets": [{"permutations": b, "rows": b * (n + 1) // 2 * 2,
                         **{c: {"rms_error": float(np.sqrt(np.mean(err2[c, b]))), "mean_se": float(np.mean(se1[c, b])),
                                "z_rms": float(np.sqrt(np.mean(z2[c, b])))} for c in controls}} for b in BUDGETS]}


def calibration_table(n, seeds, dev):
    """``error_table``'s seeds and budgets through kernelshap.pairs_se: the error, and what the bars say it should be."""
    model, data, lbl, rid, args = _setup(n, dev)
    table = exact.value_table(model, data, lbl, rid, args)
    ends = table[[0, table.numel() - 1]].cpu().numpy()
    pr = hip_ops.all_pairs(n)
    want = hip_ops.exact_interactions(table).cpu().numpy().mean(axis=1)
    most = max(BUDGETS) * (n + 1)
    err2, se2, z2, se1 = ({b: [] for b in BUDGETS} for _ in range(4))
    for seed in range(seeds):
        np.random.seed(1000 + seed)
        keep, _ = kernelshap.draw(n, most, True, dev)
        for b in BUDGETS:
            rows = keep[:b * (n + 1) // 2 * 2].contiguous()
            got, se = kernelshap.pairs_se(rows, table.index_select(0, rows).contiguous(), float(ends[0]), float(ends[1]), n)
            got, se = got[pr[:, 0], pr[:, 1]], se[pr[:, 0], pr[:, 1]]
            err2[b].append(float(((got - want) ** 2).mean()))
            se2[b].append(float((se ** 2).mean()))
            se1[b].append(float(se.mean()))
            z2[b].append(float((((got - want) / se) ** 2).mean()))
    return {"model": "pointnet", "cloud": "synthetic_00", "num_regions": n, "pairs": int(len(pr)), "seeds": seeds,
            "exact_index_rms": float(np.sqrt((want ** 2).mean())),
            "budgets": [{"permutations": b, "rows": b * (n + 1) // 2 * 2, "rms_error": float(np.sqrt(np.mean(err2[b]))),
                         "rms_se": float(np.sqrt(np.mean(se2[b]))), "mean_se": float(np.mean(se1[b])),
                         "z_rms": float(np.sqrt(np.mean(z2[b]))),
                         "per_seed_z_rms": {"min": float(np.sqrt(min(z2[b]))), "max": float(np.sqrt(max(z2[b])))}} for b in BUDGETS]}


def error_table(n, seeds, dev):
    model, data, lbl, rid, args = _setup(n, dev)
    table = exact.value_table(model, data, lbl, rid, args)
    pr = hip_ops.all_pairs(n)
    want = hip_ops.exact_interactions(table).cpu().numpy().mean(axis=1)
    most = max(BUDGETS) * (n + 1)
    sq = {b: [] for b in BUDGETS}
    for seed in range(seeds):
        np.random.seed(1000 + seed)
        keep, _ = kernelshap.draw(n, most, True, dev)
        for b in BUDGETS:
            count = b * (n + 1) // 2 * 2
            got = kernelshap.pairs_from_table(table, keep[:count].contiguous())[pr[:, 0], pr[:, 1]]
            sq[b].append(float(((got - want) ** 2).mean()))
    return {"model": "pointnet", "cloud": "synthetic_00", "num_regions": n, "pairs": int(len(pr)), "seeds": seeds,
            "exact_index_rms": float(np.sqrt((want ** 2).mean())), "exact_index_max_abs": float(np.abs(want).max()),
            "budgets": [{"permutations": b, "rows": b * (n + 1) // 2 * 2, "rms_error": float(np.sqrt(np.mean(sq[b]))),
                         "rms_error_over_exact_index_rms": float(np.sqrt(np.mean(sq[b])) / np.sqrt((want ** 2).mean())),
                         "per_seed_rms": {"mean": float(np.sqrt(sq[b]).mean()),
                                          "std": float(np.sqrt(sq[b]).std(ddof=1)) if seeds > 1 else None}} for b in BUDGETS]}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--se", action="store_true", help="time kshap_pairs_se and measure the calibration of its bars (profiles/kshap_pairs_se.json)")
    ap.add_argument("--control", action="store_true", help="the control-variate estimators: error table and time (profiles/kshap_pairs_cv.json)")
    ap.add_argument("--sparse", action="store_true", help="with --control: the sparse control alone (DESIGN.md 5k), merged into the file "
                                                         "under \"sparse\"")
    ap.add_argument("--out", default=None, help="default profiles/kshap_pairs.json, with --se profiles/kshap_pairs_se.json, with --control "
                                                "profiles/kshap_pairs_cv.json")
    ap.add_argument("--seeds", type=int, default=20)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--block", type=int, default=1 << 16, help="rows per block of the eager form")
    ap.add_argument("--error_regions", type=int, default=16)
    ap.add_argument("--games", type=int, nargs="+", default=[1, 10])
    args = ap.parse_args(argv)
    if args.se and args.control:
        ap.error("--se and --control are two runs")
    if args.sparse and not args.control:
        ap.error("--sparse belongs to --control")
    args.out = args.out or os.path.join(REPO, "profiles", "kshap_pairs_cv.json" if args.control else
                                        "kshap_pairs_se.json" if args.se else "kshap_pairs.json")
    if not torch.cuda.is_available():
        raise SystemExit("bench_kshap_pairs.py needs a GPU: a time taken elsewhere says nothing about the MI355X")
    dev = torch.device("cuda:0")
    if args.sparse:
        with torch.no_grad():
            part = {"device": torch.cuda.get_device_name(0), "time": [time_sparse(r, args.runs, dev) for r in SPARSE_REGIONS],
                    "error": sparse_table(args.error_regions, args.seeds, dev)}
        res = json.load(open(args.out)) if os.path.exists(args.out) else {}
        res["sparse"] = part
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(part))
        return
    with torch.no_grad():
        if args.control:
            timed = [time_control(r, g, args.runs, dev) for r in CONTROL_REGIONS for g in args.games]
            errors = control_table(args.error_regions, args.seeds, dev)
        else:
            timed = [time_shape(r, m, g, args.runs, args.block, dev, args.se) for r, m in SHAPES for g in args.games]
            errors = (calibration_table if args.se else error_table)(args.error_regions, args.seeds, dev)
        res = {"device": torch.cuda.get_device_name(0), "time": timed, "error": errors}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
