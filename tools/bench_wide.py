#!/usr/bin/env python3
"""Times the wide coalition path of PointNet (not the flagship workload: that is bench.py).

    python tools/bench_wide.py [--out profiles/wide_regions.json] [--repeats 5] [--perms 1000] [--regions 128 256 1024]
    python tools/bench_wide.py --profile-step 1024      # one warmed step only: the program for rocprofv3 --kernel-trace --stats

1. Wide against narrow at R = 32 (the headline's workload: 1000 permutations, 33 000 coalitions) and R = 64: the SAME coalitions
   through iq_pointnet_coalitions (the yardstick: untouched code) and iq_pointnet_coalitions_wide, alternated in one process,
   ``repeats`` times each after a warm-up of both.  Reported: coalitions/s of each run, the median ratio wide / narrow and the
   spread (max - min over median) of each side - a ratio inside the spread is no difference.  The logits are compared bitwise.
2. Coalitions/s of the wide path at R = 128, 256 and 1024 (one cloud, N = 1024, ``perms`` permutations' prefix coalitions, masks
   built on the device, launches as wide.shapley issues them), ``repeats`` runs each, median and spread.

Times are host clocks around work that ends in a device synchronise.  Kernel shares come from a separate run under the profiler
(--profile-step): tracing slows the host, so no rate is taken there."""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from interpret_quality_amd import hip_ops, synth  # noqa: E402


def _model(dev):
    from interpret_quality_amd.pointnet import PointNetCls
    model = PointNetCls(None)
    model.load_state_dict(synth.to_torch(synth.pointnet_state_dict(0)))
    return model.to(dev).eval()


def _setup(r, dev):
    pts, _ = synth.make_cloud(0)
    data = torch.from_numpy(pts).unsqueeze(0).to(dev)
    fps = hip_ops.fps(data, r)[0].contiguous()
    rid = hip_ops.region_assign_wide(data[0].contiguous(), fps).reshape(1, -1).contiguous()
    return data.contiguous(), data.mean(dim=1).reshape(1, 3).contiguous(), rid


def _orders(perms, r, dev):
    return hip_ops.as_i32(synth.make_orders(perms, r, seed=1), dev)


def _clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def _summary(rates):
    med = statistics.median(rates)
    return {"coalitions_per_s": rates, "median": med, "spread": (max(rates) - min(rates)) / med}


def wide_vs_narrow(model, r, perms, repeats, dev):
    clouds, centers, rid = _setup(r, dev)
    keep_w = hip_ops.prefix_keep_masks_wide(_orders(perms, r, dev))
    keep_n = keep_w[:, 0].contiguous()
    b = keep_w.shape[0]
    narrow = lambda: model.coalition_logits(clouds, centers, rid, keep_n, None, num_regions=r, validate=False)      # noqa: E731
    wide = lambda: model.coalition_logits_wide(clouds, centers, rid, keep_w, None, num_regions=r, validate=False)   # noqa: E731
    same = bool(torch.equal(narrow(), wide()))      # warm-up of both, and the results must not differ
    tn, tw = [], []
    for _ in range(repeats):
        tn.append(_clock(narrow)[0])
        tw.append(_clock(wide)[0])
    out = {"regions": r, "coalitions": b, "bitwise_equal": same, "narrow": _summary([b / t for t in tn]),
           "wide": _summary([b / t for t in tw])}
    out["ratio_wide_over_narrow"] = out["wide"]["median"] / out["narrow"]["median"]
    out["ratio_inside_spread"] = abs(out["ratio_wide_over_narrow"] - 1.0) <= max(out["narrow"]["spread"], out["wide"]["spread"])
    return out


def _wide_step(model, r, perms, dev):
    """One cloud's coalitions as wide.shapley issues them: masks on the device, about 2^17 coalitions per step."""
    clouds, centers, rid = _setup(r, dev)
    orders = _orders(perms, r, dev)
    step = max(1, (1 << 17) // (r + 1))

    def run():
        last = None
        for lo in range(0, perms, step):
            keep = hip_ops.prefix_keep_masks_wide(orders[lo:lo + step].contiguous())
            last = model.coalition_logits_wide(clouds, centers, rid, keep, None, num_regions=r, validate=False)
        return last
    return run, perms * (r + 1)


def wide_rate(model, r, perms, repeats, dev):
    run, b = _wide_step(model, r, perms, dev)
    run()
    times = [_clock(run)[0] for _ in range(repeats)]
    out = {"regions": r, "permutations": perms, "coalitions": b, "seconds_per_cloud": statistics.median(times)}
    out.update(_summary([b / t for t in times]))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "wide_regions.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--perms", type=int, default=1000)
    ap.add_argument("--regions", type=int, nargs="+", default=[128, 256, 1024])
    ap.add_argument("--profile-step", type=int, default=0, metavar="R",
                    help="run one warmed step at R regions and exit (the program to put under rocprofv3 --kernel-trace --stats)")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_wide.py needs a GPU: a time taken elsewhere says nothing about the MI355X")
    dev = torch.device("cuda:0")
    model = _model(dev)
    if args.profile_step:
        run, b = _wide_step(model, args.profile_step, args.perms, dev)
        run()
        t, _ = _clock(run)
        print(json.dumps({"profile_step_regions": args.profile_step, "coalitions": b, "runs": 2, "seconds_under_profiler": t}))
        return
    res = {"device": torch.cuda.get_device_name(0), "repeats": args.repeats,
           "wide_vs_narrow": [wide_vs_narrow(model, r, 1000, args.repeats, dev) for r in (32, 64)],
           "wide": [wide_rate(model, r, args.perms, args.repeats, dev) for r in args.regions]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
