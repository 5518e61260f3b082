#!/usr/bin/env python3
"""Puts the regression (KernelSHAP) estimator beside permutation sampling at equal budgets, and times its reductions (not the
flagship workload: that is bench.py).

    python tools/bench_kernelshap.py [--out profiles/kernelshap.json] [--seeds 20] [--reps 20]

Part 1 - error.  PointNet, synthetic cloud 0, n = 16 regions, ONE exact value table (65 536 coalitions).  For budgets of 100, 300
and 1000 permutations' worth of model evaluations (c (n + 1) coalitions) and ``--seeds`` seeds each, the RMS error over the
regions against the exact Shapley values of three estimators, all read off the table: permutation sampling (stage 1's estimate
of c permutations), the regression with the sampled Gram matrix and with the analytic one, both paired.  Recorded per budget:
the RMS over seeds and regions, and the ratio to permutation sampling.

Part 2 - time.  ``kshap_accum`` + ``kshap_solve`` (the Python wrappers, allocations included, as the stages call them) at
M = 33 000 rows, n = 32, for G = 1 and G = 216 games on the same rows: device events around each of ``--reps`` calls after a
warm-up, median and the 10th / 90th percentile.  Beside it the time of the PointNet forwards of the same M coalitions of n = 32
regions (``kernelshap.rewards``; G of them for G games), and the reductions' share of the two together.  The bar (DESIGN 5d's):
the reductions belong below 1 % of the forwards they follow."""
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

from interpret_quality_amd import exact, hip_ops, kernelshap, synth  # noqa: E402
from interpret_quality_amd.pointnet import PointNetCls  # noqa: E402

BUDGETS = (100, 300, 1000)      # permutations' worth of evaluations


def _setup(n, dev):
    model = PointNetCls(None)
    model.load_state_dict(synth.to_torch(synth.pointnet_state_dict(0)))
    model = model.to(dev).eval()
    pts, label = synth.make_cloud(0)
    data, lbl = torch.from_numpy(pts).unsqueeze(0).to(dev), torch.tensor([label], device=dev)
    rid = hip_ops.region_assign(data[0].contiguous(), hip_ops.fps(data, n)[0].contiguous()).cpu().numpy().astype(np.int64)
    args = SimpleNamespace(model="pointnet", softmax_type="modified", num_points=1024, num_regions=n, verbose=False)
    return model, data, lbl, rid, args


def error_table(n, seeds, dev):
    model, data, lbl, rid, args = _setup(n, dev)
    v = exact.value_table(model, data, lbl, rid, args)
    phi = hip_ops.exact_shapley(v).cpu().numpy()
    sq = {b: {"permutation": [], "sampled": [], "analytic": []} for b in BUDGETS}
    most = max(BUDGETS)
    for seed in range(seeds):
        np.random.seed(1000 + seed)
        state = hip_ops.mt_state_to_device(dev)
        orders = hip_ops.sample_permutations(state, most, n).cpu().numpy().astype(np.int64)
        hip_ops.mt_state_to_host(state, set_global=True)
        snaps, _ = exact.sampled_from_table(v, orders, list(BUDGETS))
        keep, _ = kernelshap.draw(n, most * (n + 1), True, dev)
        for b in BUDGETS:
            rows = b * (n + 1) // 2 * 2
            sq[b]["permutation"].append(((snaps[b] / b - phi) ** 2).mean())
            for gram in kernelshap.GRAMS:
                sq[b][gram].append(((kernelshap.from_table(v, keep[:rows].contiguous(), gram=gram) - phi) ** 2).mean())
    out = []
    for b in BUDGETS:
        rms = {k: float(np.sqrt(np.mean(x))) for k, x in sq[b].items()}
        out.append({"permutations": b, "evaluations": b * (n + 1), "rms_error": rms,
                    "rms_error_over_permutation": {k: rms[k] / rms["permutation"] for k in kernelshap.GRAMS}})
    return {"model": "pointnet", "cloud": "synthetic_00", "num_regions": n, "seeds": seeds,
            "phi_rms": float(np.sqrt((phi ** 2).mean())), "v_full_minus_v_empty": float(v[-1] - v[0]), "budgets": out}


def _event_times(fn, reps):
    """Device-event time of each of ``reps`` calls after two warm-up calls -> seconds, sorted."""
    fn()
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) * 1e-3)
    return sorted(times)


def _spread(times):
    return {"median_seconds": float(np.median(times)), "p10_seconds": float(np.percentile(times, 10)),
            "p90_seconds": float(np.percentile(times, 90)), "reps": len(times)}


def reduction_times(m, n, games, reps, dev):
    model, data, lbl, rid, args = _setup(n, dev)
    np.random.seed(1)
    keep, _ = kernelshap.draw(n, m, True, dev)
    kernelshap.rewards(model, data, lbl, rid, args, keep[:1024].contiguous())       # warm-up: engine, workspace, code objects
    torch.cuda.synchronize()
    fwd = []
    for _ in range(3):
        t0 = time.perf_counter()
        v, v_full, v_empty = kernelshap.rewards(model, data, lbl, rid, args, keep)
        torch.cuda.synchronize()
        fwd.append(time.perf_counter() - t0)
    forward = float(np.median(fwd))
    out = {"rows": int(keep.numel()), "num_regions": n, "pointnet_forwards": {"median_seconds": forward, "runs": fwd,
                                                                               "coalitions_per_s": (keep.numel() + 2) / forward}}
    rng = np.random.default_rng(2)
    for g in games:
        # G games on the same rows: game 0 is the cloud's own, the others seeded perturbations of it (only the shape matters here)
        vg = (v[None, :] * torch.from_numpy(1.0 + 0.01 * rng.standard_normal((g, 1)).astype(np.float32)).to(dev)).contiguous()
        v0 = torch.full((g,), v_empty, dtype=torch.float64, device=dev)
        delta = torch.full((g,), v_full - v_empty, dtype=torch.float64, device=dev)

        def reduce():
            a, b, w = hip_ops.kshap_accum(keep, vg, v0, n)
            return hip_ops.kshap_solve((a / w).contiguous(), (b / w).contiguous(), delta)

        def accum_only():
            return hip_ops.kshap_accum(keep, vg, v0, n)

        both, acc = _event_times(reduce, reps), _event_times(accum_only, reps)
        red = float(np.median(both))
        out["G=%d" % g] = {"accum_and_solve": _spread(both), "accum_alone": _spread(acc), "forwards_seconds": forward * g,
                           "reductions_share_of_forwards_plus_reductions": red / (red + forward * g),
                           "float64_fma": int(keep.numel()) * n * (n + g)}
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "kernelshap.json"))
    ap.add_argument("--seeds", type=int, default=20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--error_regions", type=int, default=16)
    ap.add_argument("--rows", type=int, default=33000)
    ap.add_argument("--time_regions", type=int, default=32)
    ap.add_argument("--games", type=int, nargs="+", default=[1, 216])
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_kernelshap.py needs a GPU: a time taken elsewhere says nothing about the MI355X")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0),
           "error": error_table(args.error_regions, args.seeds, dev),
           "time": reduction_times(args.rows, args.time_regions, args.games, args.reps, dev)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
