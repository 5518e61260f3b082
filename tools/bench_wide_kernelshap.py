#!/usr/bin/env python3
"""Puts the wide regression (KernelSHAP) estimator beside permutation sampling at equal budgets, and times its three parts (not
the flagship workload: that is bench.py).

    python tools/bench_wide_kernelshap.py [--out profiles/wide_kernelshap.json] [--seeds 20] [--runs 5] [--draw]

Part 1 - error.  PointNet, synthetic cloud 0, R = 128 regions.  There is no exact value at this size, so the yardstick is a long
permutation run of its own seed (``--long`` = 20 000 permutations through ``wide.shapley``), with its standard error per region
(the standard deviation of the per-permutation marginals over sqrt(count)) reported beside it.  For budgets of 100, 300 and 1000
permutations' worth of model evaluations (c (R + 1) coalitions) and ``--seeds`` seeds each: the RMS difference to the yardstick
over regions and seeds of ``wide.shapley``'s estimate of c permutations and of ``wide_kernelshap``'s of c (R + 1) rows (paired), the
ratio of the two, and per estimator the mean and standard deviation over seeds of the per-seed RMS.  ``difference_counts`` is true
only where the two RMS values differ by more than the yardstick's standard error AND by more than the spread over seeds of the
per-seed difference.  Both estimators' RMS include the yardstick's own error in quadrature.

Part 2 - time.  R = 128 and 1024, M = 1000 (R + 1) rows, ``--runs`` runs each after a warm-up, wall clock around a synchronised
call, median and the smallest and largest run: the draw (sizes on the host, permutations on the device, keep rows:
``wide_kernelshap.draw``), the PointNet forwards of those rows (``wide_kernelshap.rewards``), and moment + phi
(``hip_ops.kshap_moment_wide`` + ``hip_ops.kshap_phi_analytic``, the wrappers with their allocations).  Shares: moment + phi in
forwards plus moment + phi (DESIGN 5f's yardstick: below 1 %), and the draw in the sum of all three.

``--draw`` - the counter-based draw (``wide_kernelshap.draw_counter``) beside the stream draw; the file at ``--out`` keeps its
"time" and gains two things.  Error: part 1 again, same yardstick, same seeds, with a third estimator column "kernelshap_counter",
the same estimator on counter-drawn rows (key: the seed, stream 0), and its ratios to the other two.  Time ("draw_time"): at each
region count the two draws of M = 1000 (R + 1) rows ALTERNATED in one process, ``--runs`` each after one full warm-up call of
each, median and smallest-to-largest spread, whether the difference of the medians exceeds the larger spread, and the forwards and
reductions of the same rows timed in the same process, for each draw's share of draw + forwards + reductions."""
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

from interpret_quality_amd import hip_ops, synth, wide, wide_kernelshap  # noqa: E402
from interpret_quality_amd.pointnet import PointNetCls  # noqa: E402

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


def _orders(count, r, dev):
    state = hip_ops.mt_state_to_device(dev)
    orders = hip_ops.sample_permutations_wide(state, count, r).cpu().numpy().astype(np.int64)
    hip_ops.mt_state_to_host(state, set_global=True)
    return orders


def error_table(r, seeds, long_run, dev, counter=False):
    model, data, lbl, rid, args = _setup(r, dev)
    np.random.seed(987654)
    _, rows, total = wide.shapley(model, data, lbl, rid, _orders(long_run, r, dev), args)
    yard = total / long_run
    se = rows.std(axis=0, ddof=1) / np.sqrt(long_run)
    most = max(BUDGETS)
    sq = {b: {k: [] for k in ("permutation", "kernelshap") + (("kernelshap_counter",) if counter else ())} for b in BUDGETS}
    for seed in range(seeds):
        np.random.seed(1000 + seed)
        snaps, _, _ = wide.shapley(model, data, lbl, rid, _orders(most, r, dev), args, snap_counts=list(BUDGETS))
        counts = [b * (r + 1) for b in BUDGETS]
        _, _, _, running = wide_kernelshap.shapley(model, data, lbl, rid, args, samples=most * (r + 1), counts=counts)
        for b in BUDGETS:
            sq[b]["permutation"].append(float(((snaps[b] / b - yard) ** 2).mean()))
            sq[b]["kernelshap"].append(float(((running[b * (r + 1) // 2 * 2] - yard) ** 2).mean()))
        if counter:
            _, _, _, running = wide_kernelshap.shapley(model, data, lbl, rid, args, samples=most * (r + 1), counts=counts, draw="counter",
                                                       seed=1000 + seed, stream=0)
            for b in BUDGETS:
                sq[b]["kernelshap_counter"].append(float(((running[b * (r + 1) // 2 * 2] - yard) ** 2).mean()))
    se_rms = float(np.sqrt((se ** 2).mean()))
    out = []
    for b in BUDGETS:
        per_seed = {k: np.sqrt(np.array(x)) for k, x in sq[b].items()}
        rms = {k: float(np.sqrt(np.mean(x))) for k, x in sq[b].items()}
        diff = per_seed["kernelshap"] - per_seed["permutation"]
        spread = float(diff.std(ddof=1)) if seeds > 1 else float("inf")
        gap = abs(rms["kernelshap"] - rms["permutation"])
        out.append({"permutations": b, "evaluations": b * (r + 1), "rms_difference_to_yardstick": rms,
                    "kernelshap_over_permutation": rms["kernelshap"] / rms["permutation"],
                    "per_seed_rms": {k: {"mean": float(x.mean()), "std": float(x.std(ddof=1)) if seeds > 1 else None}
                                     for k, x in per_seed.items()},
                    "per_seed_difference_std": spread, "difference_counts": bool(gap > se_rms and gap > spread)})
        if counter:
            diff = per_seed["kernelshap_counter"] - per_seed["kernelshap"]
            spread = float(diff.std(ddof=1)) if seeds > 1 else float("inf")
            gap = abs(rms["kernelshap_counter"] - rms["kernelshap"])
            out[-1].update({"counter_over_permutation": rms["kernelshap_counter"] / rms["permutation"],
                            "counter_over_kernelshap": rms["kernelshap_counter"] / rms["kernelshap"],
                            "counter_per_seed_difference_std": spread, "counter_difference_counts": bool(gap > se_rms and gap > spread)})
    return {"model": "pointnet", "cloud": "synthetic_00", "num_regions": r, "seeds": seeds,
            "yardstick": {"permutations": long_run, "seed": 987654, "standard_error_rms": se_rms, "standard_error_max": float(se.max()),
                          "phi_rms": float(np.sqrt((yard ** 2).mean()))},
            "budgets": out}


def _wall(fn, runs):
    """Wall-clock seconds of each of ``runs`` synchronised calls -> (list, the last call's result)."""
    times, res = [], None
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return times, res


def _spread(times):
    return {"median_seconds": float(np.median(times)), "min_seconds": float(min(times)), "max_seconds": float(max(times)),
            "runs": [float(t) for t in times]}


def part_times(r, runs, dev):
    model, data, lbl, rid, args = _setup(r, dev)
    m = 1000 * (r + 1) // 2 * 2
    np.random.seed(1)
    warm, _ = wide_kernelshap.draw(r, 2048, True, dev)
    wide_kernelshap.rewards(model, data, lbl, rid, args, warm)          # warm-up: engine, workspace, code objects
    draw, (keep, _) = _wall(lambda: wide_kernelshap.draw(r, m, True, dev), runs)
    fwd, (v, v_full, v_empty) = _wall(lambda: wide_kernelshap.rewards(model, data, lbl, rid, args, keep), runs)
    v2 = v.reshape(1, -1).contiguous()
    v0 = torch.tensor([v_empty], dtype=torch.float64, device=dev)
    delta = torch.tensor([v_full - v_empty], dtype=torch.float64, device=dev)

    def reduce():
        b, w = hip_ops.kshap_moment_wide(keep, v2, v0, r)
        return hip_ops.kshap_phi_analytic(b, w, delta)

    reduce()
    red, _ = _wall(reduce, runs)
    d, f, s = float(np.median(draw)), float(np.median(fwd)), float(np.median(red))
    return {"num_regions": r, "rows": int(keep.shape[0]), "draw": _spread(draw), "pointnet_forwards": _spread(fwd),
            "coalitions_per_s": (keep.shape[0] + 2) / f, "moment_and_phi": _spread(red),
            "moment_and_phi_share_of_forwards_plus_reductions": s / (f + s), "draw_share_of_total": d / (d + f + s)}


def draw_times(r, runs, dev):
    """The stream draw and the counter draw of M = 1000 (R + 1) rows, alternated, then the forwards and reductions of those rows."""
    model, data, lbl, rid, args = _setup(r, dev)
    m = 1000 * (r + 1) // 2 * 2
    np.random.seed(1)
    wide_kernelshap.draw(r, m, True, dev)                               # warm-up: one full call of each
    keep, _ = wide_kernelshap.draw_counter(r, m, 1, 0, True, dev)
    stream, counter = [], []
    for _ in range(runs):
        stream += _wall(lambda: wide_kernelshap.draw(r, m, True, dev), 1)[0]
        counter += _wall(lambda: wide_kernelshap.draw_counter(r, m, 1, 0, True, dev), 1)[0]
    wide_kernelshap.rewards(model, data, lbl, rid, args, keep[:4096].contiguous())
    fwd, (v, v_full, v_empty) = _wall(lambda: wide_kernelshap.rewards(model, data, lbl, rid, args, keep), runs)
    v2 = v.reshape(1, -1).contiguous()
    v0 = torch.tensor([v_empty], dtype=torch.float64, device=dev)
    delta = torch.tensor([v_full - v_empty], dtype=torch.float64, device=dev)

    def reduce():
        b, w = hip_ops.kshap_moment_wide(keep, v2, v0, r)
        return hip_ops.kshap_phi_analytic(b, w, delta)

    reduce()
    red, _ = _wall(reduce, runs)
    ds, dc, f, s = (float(np.median(x)) for x in (stream, counter, fwd, red))
    larger_spread = max(max(stream) - min(stream), max(counter) - min(counter))
    return {"num_regions": r, "rows": int(keep.shape[0]), "stream_draw": _spread(stream), "counter_draw": _spread(counter),
            "stream_over_counter": ds / dc, "larger_spread_seconds": larger_spread,
            "counter_faster_by_more_than_the_larger_spread": bool(ds - dc > larger_spread),
            "pointnet_forwards": _spread(fwd), "moment_and_phi": _spread(red),
            "stream_draw_share_of_total": ds / (ds + f + s), "counter_draw_share_of_total": dc / (dc + f + s)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "wide_kernelshap.json"))
    ap.add_argument("--seeds", type=int, default=20)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--long", type=int, default=20000)
    ap.add_argument("--error_regions", type=int, default=128)
    ap.add_argument("--time_regions", type=int, nargs="+", default=[128, 1024])
    ap.add_argument("--draw", action="store_true", help="the counter-based draw beside the stream draw: error column and alternated times")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_wide_kernelshap.py needs a GPU: a time taken elsewhere says nothing about the MI355X")
    dev = torch.device("cuda:0")
    if args.draw:
        res = json.load(open(args.out)) if os.path.exists(args.out) else {"device": torch.cuda.get_device_name(0)}
        res["error"] = error_table(args.error_regions, args.seeds, args.long, dev, counter=True)
        res["draw_time"] = [draw_times(r, args.runs, dev) for r in args.time_regions]
    else:
        res = {"device": torch.cuda.get_device_name(0),
               "error": error_table(args.error_regions, args.seeds, args.long, dev),
               "time": [part_times(r, args.runs, dev) for r in args.time_regions]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
