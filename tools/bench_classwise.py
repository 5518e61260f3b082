#!/usr/bin/env python3
"""Times the all-class reductions beside the single-label ones they replace (not the flagship workload: that is bench.py).

    python tools/bench_classwise.py [--out profiles/classwise.json] [--runs 5] [--regions 32 1024] [--permutations 1000]

PointNet, synthetic cloud 0, R = 32 (a narrow game) and R = 1024 (one region per point), 1000 permutations, G = C classes of the
synthetic model.  The logits of the S (R + 1) prefix coalitions are evaluated once (final_common.shapley_logits up to 64 regions,
wide.shapley's steps above) and kept; on those rows, ``--runs`` runs each after a warm-up, wall clock around a synchronised call
of the wrappers with their allocations, median and smallest-to-largest spread:

* ``classes``        hip_ops.reward_classes + hip_ops.shapley_accum_games (all G games),
* ``single``         hip_ops.reward + hip_ops.shapley_accum[_wide] once (one game: what stage 1 does today),
* ``single_g_times`` that pair run G times (the only route to G games before),

each also as a share of the time of those rows' forwards (``forwards``: the same number of runs), and the float64 row tables the
single-label route holds for G games against the games route's scratch.  Recorded numbers, not gates."""
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

from interpret_quality_amd import final_common, hip_ops, synth, wide  # noqa: E402
from interpret_quality_amd.pointnet import PointNetCls  # noqa: E402


def _setup(r, dev):
    model = PointNetCls(None)
    model.load_state_dict(synth.to_torch(synth.pointnet_state_dict(0)))
    model = model.to(dev).eval()
    pts, label = synth.make_cloud(0)
    data = torch.from_numpy(pts).unsqueeze(0).to(dev)
    rid = hip_ops.region_assign_wide(data[0].contiguous(), hip_ops.fps(data, r)[0].contiguous()).cpu().numpy().astype(np.int64)
    args = SimpleNamespace(model="pointnet", softmax_type="modified", num_points=1024, num_regions=r, verbose=False)
    return model, data, int(label), rid, args


def _wall(fn, runs):
    times, res = [], None
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return times, res


def _spread(times, forwards=None):
    out = {"median_seconds": float(np.median(times)), "min_seconds": float(min(times)), "max_seconds": float(max(times)),
           "runs": [float(t) for t in times]}
    if forwards is not None:
        out["share_of_forwards"] = out["median_seconds"] / forwards
    return out


def one_game(r, s, runs, dev):
    model, data, label, rid, args = _setup(r, dev)
    rng = np.random.RandomState(1)
    orders = np.stack([rng.permutation(r) for _ in range(s)])
    orders_dev = hip_ops.as_i32(orders, dev)
    rid_dev = hip_ops.region_ids(rid, dev, r)

    def forwards():
        with torch.no_grad():
            if r <= 64:
                return final_common.shapley_logits(model, data, None, rid, orders, args)
            return torch.cat([wide._prefix_logits(model, data, rid_dev, step, r) for _, _, step in wide._steps(orders_dev, r)])

    forwards()                                            # warm-up: engine, workspace, code objects
    fwd, logits = _wall(forwards, runs)
    logits = logits.contiguous()
    c = logits.shape[1]
    accum = hip_ops.shapley_accum if r <= 64 else hip_ops.shapley_accum_wide

    def classes():
        return hip_ops.shapley_accum_games(hip_ops.reward_classes(logits, None, True), orders_dev, validate=False)[0]

    def single(lab=label):
        return accum(hip_ops.reward(logits, lab, True), orders_dev)[0]

    def single_g_times():
        return torch.stack([single(lab) for lab in range(c)])

    assert torch.equal(classes().view(torch.int64), single_g_times().view(torch.int64))     # the same bits, before anything is timed
    f = float(np.median(fwd))
    times = {name: _spread(_wall(fn, runs)[0], f) for name, fn in (("classes", classes), ("single", single), ("single_g_times", single_g_times))}
    return {"num_regions": r, "permutations": s, "coalitions": s * (r + 1), "classes": c, "forwards": _spread(fwd), **times,
            "classes_over_single": times["classes"]["median_seconds"] / times["single"]["median_seconds"],
            "single_g_times_over_classes": times["single_g_times"]["median_seconds"] / times["classes"]["median_seconds"],
            "row_table_bytes_single_route_g_games": c * s * r * 8, "games_scratch_bytes": hip_ops.shapley_games_scratch_bytes(r, s, c)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "classwise.json"))
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--regions", type=int, nargs="+", default=[32, 1024])
    ap.add_argument("--permutations", type=int, default=1000)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_classwise.py needs a GPU: a time taken elsewhere says nothing about the MI355X")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "model": "pointnet", "cloud": "synthetic_00", "runs": args.runs,
           "games": [one_game(r, args.permutations, args.runs, dev) for r in args.regions]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
