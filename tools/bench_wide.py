#!/usr/bin/env python3
"""Times the wide coalition path of PointNet (not the flagship workload: that is bench.py).

    python tools/bench_wide.py [--out profiles/wide_regions.json] [--repeats 5] [--perms 1000] [--regions 128 256 1024]
    python tools/bench_wide.py --profile-step 1024 [--route keep|prefix]   # one warmed step only: the program for rocprofv3 --kernel-trace --stats
    python tools/bench_wide.py --prefix                 # wide.shapley, keep route against prefix route, into the "prefix" key of --out
    python tools/bench_wide.py --interaction            # the interaction stage only, into the "interaction" key of --out
    python tools/bench_wide.py --compact                # the other families, dense against compact, into the "compact" key of --out
    python tools/bench_wide.py --poses                  # a pose sweep, one wide.shapley per pose against wide.shapley_over_poses, into "poses"
    python tools/bench_wide.py --sampler                # the draws of a wide game, host against device, into the "sampler" key of --out
    python tools/bench_wide.py --profile-sampler 1024   # one warmed device draw of one ratio only: the program for rocprofv3 --kernel-trace --stats

1. Wide against narrow at R = 32 (the headline's workload: 1000 permutations, 33 000 coalitions) and R = 64: the SAME coalitions
   through iq_pointnet_coalitions (the yardstick: untouched code) and iq_pointnet_coalitions_wide, alternated in one process,
   ``repeats`` times each after a warm-up of both.  Reported: coalitions/s of each run, the median ratio wide / narrow and the
   spread (max - min over median) of each side - a ratio inside the spread is no difference.  The logits are compared bitwise.
2. Coalitions/s of the wide path at R = 128, 256 and 1024 (one cloud, N = 1024, ``perms`` permutations' prefix coalitions, masks
   built on the device, launches as wide.shapley issues them), ``repeats`` runs each, median and spread.

3. ``--interaction``: (a) one ratio of the wide interaction stage as final_wide_interaction.py issues it - 300 pairs x 100 contexts
   at ratio 0.5 (120 000 coalitions) through wide.interaction_logits at R = 128 and R = 1024, contexts drawn by wide.gen_context:
   coalitions/s, and the seconds of the mask kernel alone; (b) the wide route against the narrow stage
   (interaction.compute_order_interaction_logits: untouched code) on identical pairs and contexts at R = 64, alternated in one
   process, ratio and spread as in 1.  Both routes hand the chain kernels the same row lists, so the expectation is a ratio inside
   the spread (the narrow route also de-duplicates on the host; sampled contexts of 31 regions out of 62 do not repeat).

4. ``--prefix``: wide.shapley on one synthetic cloud at R = 128, 256 and 1024 (N = 1024), route="keep" (the yardstick: the parent's
   code path, untouched) against route="prefix" (iq_pointnet_prefix_coalitions_wide), alternated in one process after a warm-up of
   both, ``repeats`` runs each (at least five), with as many whole steps of permutations as make a run about a second.  Reported per
   R: seconds and coalitions/s of every run, median and spread of each route, the ratio of the medians, whether the Shapley rows are
   the same bits, and ``prefix_slower_beyond_spread`` - the one condition under which wide.DEFAULT_ROUTE must be "keep".

5. ``--compact``: the other families (pointnet2, dgcnn, gcnn, pointconv; ``--families``) - wide.shapley on one synthetic cloud,
   N = 1024, at R = 128 and R = 1024, coalitions="dense" (the yardstick: the parent's code path, untouched - masked clouds into the
   dense forward) against coalitions="compact" (the iq_*_coalitions_wide entries), alternated in one process after one warm-up of
   both, five runs each, with as many whole permutations as make a dense run about a second.  Reported per family and R: seconds
   and coalitions/s of every run, median and spread of each route, the ratio of the medians, ``compact_faster_beyond_spread`` and
   the norm-wise difference of the Shapley rows.  Into the "compact" key of --out.  No threshold hangs on these numbers.

6. ``--poses``: PointNet, N = 1024, R = 128 and R = 1024, S = 100 permutations, P = 32 rotations of one synthetic cloud (6.6 k to
   102 k coalitions a pose: the shape of final_wide_pose.py).  Arm (a), the yardstick: P separate calls of wide.shapley - the
   parent's code path, not the code under test.  Arm (b): wide.shapley_over_poses.
   Alternated in one process after a warm-up of both, five runs each.  Reported per R: seconds and coalitions/s of every run,
   median and spread of each arm, whether the values are the same bits, and ``batched_slower_beyond_spread`` /
   ``batched_faster`` - batching poses across launches stays only if it is slower beyond the larger spread at neither region
   count and faster at one of them (``batching_stays_by_the_rule``).  Into the "poses" key of --out.

7. ``--sampler``: the random draws of a wide game, NumPy's global generator on the host (the yardstick: the parent's code path,
   untouched) against the same stream on the device (iq_sample_permutations_wide), alternated in one process after a warm-up of
   both, five runs each, every side up to and including the host array the driver saves.  (a) One ratio of the interaction
   driver's default job - 300 pairs x 100 contexts at ratio 0.5, an int16 array - at R = 128 and R = 1024 through
   wide.iter_contexts; (b) the same ratio passed over, as for a cloud that is not selected: the host has no way to pass a draw
   over but to draw it, the device runs wide.skip_contexts; (c) stage 1's 1000 permutations at R = 1024 through
   wide_stage.generate_all_orders (an int64 array).  Reported per leg: seconds of every run, median and spread of each side, the
   ratio of the medians, ``device_faster_beyond_spread`` and whether both sides gave the same bits from the same seed.  Into the
   "sampler" key of --out.  No threshold hangs on these numbers and the drivers' default stays ``--sampler host``.

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


def _wide_step(model, r, perms, dev, route="keep"):
    """One cloud's coalitions as wide.shapley issues them, about 2^17 coalitions per step: masks on the device and arbitrary wide
    coalitions (``route`` "keep"), or straight from the permutations ("prefix")."""
    clouds, centers, rid = _setup(r, dev)
    orders = _orders(perms, r, dev)
    step = max(1, (1 << 17) // (r + 1))

    def run():
        last = None
        for lo in range(0, perms, step):
            o = orders[lo:lo + step].contiguous()
            if route == "prefix":
                last = model.prefix_logits_wide(clouds, centers, rid, o, None, num_regions=r, validate=False)
            else:
                last = model.coalition_logits_wide(clouds, centers, rid, hip_ops.prefix_keep_masks_wide(o), None, num_regions=r,
                                                   validate=False)
        return last
    return run, perms * (r + 1)


def wide_rate(model, r, perms, repeats, dev):
    run, b = _wide_step(model, r, perms, dev)
    run()
    times = [_clock(run)[0] for _ in range(repeats)]
    out = {"regions": r, "permutations": perms, "coalitions": b, "seconds_per_cloud": statistics.median(times)}
    out.update(_summary([b / t for t in times]))
    return out


def prefix_vs_keep(model, r, repeats, dev, min_seconds=1.0):
    """wide.shapley on one cloud, route "keep" against route "prefix", alternated; see the module docstring, 4."""
    import math
    from interpret_quality_amd import wide
    data, _, rid = _setup(r, dev)
    rid_np = rid[0].cpu().numpy().astype(np.int64)
    lbl = torch.zeros((1,), dtype=torch.int64, device=dev)
    args = argparse.Namespace(model="pointnet", softmax_type="modified", num_points=1024, num_regions=r, verbose=False)
    step = max(1, (1 << 17) // (r + 1))
    run = lambda route, orders: wide.shapley(model, data, lbl, rid_np, orders, args, route=route)      # noqa: E731
    one = synth.make_orders(step, r, seed=1)
    for route in wide.ROUTES:                      # warm-up of both at the step's shape
        run(route, one)
    t_step = min(_clock(lambda: run(route, one))[0] for route in wide.ROUTES)
    perms = step * max(1, math.ceil(min_seconds / t_step))       # whole steps, about a second for the faster route
    orders = synth.make_orders(perms, r, seed=1)
    same = bool(np.array_equal(run("keep", orders)[1], run("prefix", orders)[1]))     # second warm-up; the results must not differ
    times = {route: [] for route in wide.ROUTES}
    for _ in range(max(5, repeats)):
        for route in ("keep", "prefix"):
            times[route].append(_clock(lambda: run(route, orders))[0])
    b = perms * (r + 1)
    out = {"regions": r, "permutations": perms, "coalitions": b, "rows_bitwise_equal": same}
    for route in wide.ROUTES:
        out[route] = dict(_summary([b / t for t in times[route]]), seconds=times[route], median_seconds=statistics.median(times[route]))
    keep, prefix = out["keep"], out["prefix"]
    out["ratio_prefix_over_keep"] = prefix["median"] / keep["median"]
    out["prefix_slower_beyond_spread"] = (keep["median"] - prefix["median"]) / keep["median"] > max(keep["spread"], prefix["spread"])
    return out


def poses_batched_vs_looped(model, r, dev, perms=100, n_poses=32, repeats=5):
    """A pose sweep, one wide.shapley call per pose against wide.shapley_over_poses, alternated; see the module docstring, 6."""
    from interpret_quality_amd import pose_sweep, wide
    data, _, rid = _setup(r, dev)
    rid_np = rid[0].cpu().numpy().astype(np.int64)
    lbl = torch.zeros((1,), dtype=torch.int64, device=dev)
    args = argparse.Namespace(model="pointnet", softmax_type="modified", num_points=1024, num_regions=r, verbose=False,
                              angle_threshold=pose_sweep.ANGLE_THRESHOLD, num_grid_enum_rotate=pose_sweep.NUM_GRID_ENUM_ROTATE)
    angles = pose_sweep.generate_rotate_angle(args, dev)[:n_poses]
    poses = torch.cat([pose_sweep.rotate_xyz(data, angles[i]) for i in range(n_poses)], dim=0).contiguous()
    orders = synth.make_orders(perms, r, seed=1)
    looped = lambda: np.stack([wide.shapley(model, poses[k:k + 1], lbl, rid_np, orders, args)[2] / perms for k in range(n_poses)])  # noqa: E731
    batched = lambda: wide.shapley_over_poses(model, poses, lbl, rid_np, orders, args).cpu().numpy()                                # noqa: E731
    same = bool(np.array_equal(looped(), batched()))      # warm-up of both, and the results must not differ
    times = {"looped": [], "batched": []}
    for _ in range(repeats):
        times["looped"].append(_clock(looped)[0])
        times["batched"].append(_clock(batched)[0])
    b = n_poses * perms * (r + 1)
    out = {"regions": r, "poses": n_poses, "permutations": perms, "coalitions": b, "values_bitwise_equal": same}
    for arm in times:
        out[arm] = dict(_summary([b / t for t in times[arm]]), seconds=times[arm], median_seconds=statistics.median(times[arm]))
    a, bt = out["looped"], out["batched"]
    out["ratio_batched_over_looped"] = bt["median"] / a["median"]
    out["batched_slower_beyond_spread"] = (a["median"] - bt["median"]) / a["median"] > max(a["spread"], bt["spread"])
    out["batched_faster"] = bt["median"] > a["median"]
    return out


COMPACT_FAMILIES = ("pointnet2", "dgcnn", "gcnn", "pointconv")


def _family_model(family, dev):
    ns = argparse.Namespace(dataset="modelnet10", k=20)
    if family == "pointnet2":
        from interpret_quality_amd.pointnet2 import PointNet2ClsMsg
        model, sd = PointNet2ClsMsg(None), synth.pointnet2_state_dict(0)
    elif family == "pointconv":
        from interpret_quality_amd.pointconv import PointConvDensityClsSsg
        model, sd = PointConvDensityClsSsg(None), synth.pointconv_state_dict(0)
    else:
        from interpret_quality_amd.dgcnn import DGCNN_cls, GCNN_cls
        model, sd = (DGCNN_cls if family == "dgcnn" else GCNN_cls)(ns), synth.dgcnn_state_dict(0)
    model.load_state_dict(synth.to_torch(sd))
    return model.to(dev).eval()


def compact_vs_dense(family, model, r, repeats, dev, min_seconds=1.0):
    """wide.shapley on one cloud, coalitions "dense" against "compact", alternated; see the module docstring, 5."""
    import math
    from interpret_quality_amd import wide
    data, _, rid = _setup(r, dev)
    rid_np = rid[0].cpu().numpy().astype(np.int64)
    lbl = torch.zeros((1,), dtype=torch.int64, device=dev)
    args = argparse.Namespace(model=family, softmax_type="modified", num_points=1024, num_regions=r, verbose=False)
    run = lambda mode, orders: wide.shapley(model, data, lbl, rid_np, orders, args, coalitions=mode)      # noqa: E731
    one = synth.make_orders(1, r, seed=1)
    run("dense", one)                              # sizing: a warmed dense run of one permutation
    t_perm = _clock(lambda: run("dense", one))[0]
    perms = max(1, math.ceil(min_seconds / t_perm))
    orders = synth.make_orders(perms, r, seed=1)
    rows = {mode: run(mode, orders)[1] for mode in wide.COALITIONS}      # the one warm-up of both routes at the run's shape
    diff = float(np.linalg.norm(rows["compact"] - rows["dense"]) / max(np.linalg.norm(rows["dense"]), 1e-300))
    times = {mode: [] for mode in wide.COALITIONS}
    for _ in range(repeats):
        for mode in wide.COALITIONS:
            times[mode].append(_clock(lambda: run(mode, orders))[0])
    b = perms * (r + 1)
    out = {"family": family, "regions": r, "points": 1024, "permutations": perms, "coalitions": b, "rows_rel_norm_diff": diff}
    for mode in wide.COALITIONS:
        out[mode] = dict(_summary([b / t for t in times[mode]]), seconds=times[mode], median_seconds=statistics.median(times[mode]))
    dense, compact = out["dense"], out["compact"]
    out["ratio_compact_over_dense"] = compact["median"] / dense["median"]
    out["compact_faster_beyond_spread"] = (compact["median"] - dense["median"]) / dense["median"] > max(dense["spread"], compact["spread"])
    return out


def _interaction_inputs(r, pairs_n, ctx_n, ratio):
    from interpret_quality_amd import wide
    np.random.seed(1)
    pairs = wide.gen_pair_random(argparse.Namespace(num_regions=r, num_pairs_random=pairs_n))
    return pairs, wide.gen_context(pairs, r, [ratio], ctx_n)[0]


def _interaction_args(r):
    return argparse.Namespace(model="pointnet", softmax_type="modified", num_points=1024, num_regions=r, interaction_batch_size=25)


def interaction_rate(model, r, repeats, dev, pairs_n=300, ctx_n=100, ratio=0.5):
    from interpret_quality_amd import wide
    data, _, rid = _setup(r, dev)
    rid_np = rid[0].cpu().numpy().astype(np.int64)
    pairs, ctx = _interaction_inputs(r, pairs_n, ctx_n, ratio)
    args = _interaction_args(r)
    run = lambda: wide.interaction_logits(model, data, rid_np, pairs, ctx, args)      # noqa: E731
    run()
    times = [_clock(run)[0] for _ in range(repeats)]
    pd, cd = hip_ops.as_i32(pairs, dev), hip_ops.as_i32(ctx, dev)
    masks = lambda: hip_ops.context_keep_masks_wide(pd, cd, r)                        # noqa: E731
    masks()
    mask_times = [_clock(masks)[0] for _ in range(repeats)]
    b = 4 * ctx.shape[0] * ctx.shape[1]
    out = {"regions": r, "pairs": int(ctx.shape[0]), "contexts": int(ctx.shape[1]), "context_regions": int(ctx.shape[2]), "coalitions": b,
           "seconds_per_ratio": statistics.median(times), "mask_kernel_seconds": statistics.median(mask_times)}
    out.update(_summary([b / t for t in times]))
    return out


def interaction_wide_vs_narrow(model, repeats, dev, r=64, pairs_n=300, ctx_n=100, ratio=0.5):
    import contextlib
    import io
    from interpret_quality_amd import interaction, wide
    data, _, rid = _setup(r, dev)
    rid_np = rid[0].cpu().numpy().astype(np.int64)
    pairs, ctx = _interaction_inputs(r, pairs_n, ctx_n, ratio)
    args = _interaction_args(r)

    def narrow():
        with contextlib.redirect_stdout(io.StringIO()):
            return interaction.compute_order_interaction_logits(model, data, rid_np, pairs, ctx, args)
    wide_run = lambda: wide.interaction_logits(model, data, rid_np, pairs, ctx, args)  # noqa: E731
    same = bool(torch.equal(narrow(), wide_run()))      # warm-up of both, and the results must not differ
    tn, tw = [], []
    for _ in range(repeats):
        tn.append(_clock(narrow)[0])
        tw.append(_clock(wide_run)[0])
    b = 4 * ctx.shape[0] * ctx.shape[1]
    out = {"regions": r, "coalitions": b, "bitwise_equal": same, "narrow": _summary([b / t for t in tn]),
           "wide": _summary([b / t for t in tw])}
    out["ratio_wide_over_narrow"] = out["wide"]["median"] / out["narrow"]["median"]
    out["ratio_inside_spread"] = abs(out["ratio_wide_over_narrow"] - 1.0) <= max(out["narrow"]["spread"], out["wide"]["spread"])
    return out


def _seconds(ts):
    med = statistics.median(ts)
    return {"seconds": ts, "median": med, "spread": (max(ts) - min(ts)) / med}


def _host_vs_device(name, host, device, repeats, same):
    """``host`` and ``device`` alternated after a warm-up of both; ``same(a, b)``: the two results from one seed are the same bits."""
    np.random.seed(1)
    a = host()
    np.random.seed(1)
    b = device()
    th, td = [], []
    for _ in range(repeats):
        th.append(_clock(host)[0])
        td.append(_clock(device)[0])
    out = {"leg": name, "host": _seconds(th), "device": _seconds(td), "same_bits": bool(same(a, b))}
    out["ratio_host_over_device"] = out["host"]["median"] / out["device"]["median"]
    out["device_faster_beyond_spread"] = out["ratio_host_over_device"] - 1.0 > max(out["host"]["spread"], out["device"]["spread"])
    return out


def _sampler_ratio(r, dev, pairs_n=300, ctx_n=100, ratio=0.5):
    """One ratio of final_wide_interaction.py's default draw at R regions -> (host, device, device skip) callables."""
    from interpret_quality_amd import wide
    from interpret_quality_amd.wide_interaction_stage import CONTEXT_DTYPE
    np.random.seed(0)
    pairs = wide.gen_pair_random(argparse.Namespace(num_regions=r, num_pairs_random=pairs_n))

    def draw(device):
        return next(iter(wide.iter_contexts(pairs, r, [ratio], ctx_n, dtype=CONTEXT_DTYPE, device=device)))
    return (lambda: draw(None)), (lambda: draw(dev)), (lambda: wide.skip_contexts(pairs_n, r, [ratio], ctx_n, dev))


def sampler_host_vs_device(repeats, dev, regions=(128, 1024), perms=1000):
    from interpret_quality_amd import wide_stage
    legs = []
    for r in regions:
        host, device, skip = _sampler_ratio(r, dev)
        leg = _host_vs_device("one ratio: 300 pairs x 100 contexts, ratio 0.5", host, device, repeats,
                              lambda a, b: a.dtype == b.dtype and np.array_equal(a, b))
        legs.append(dict(leg, regions=r, permutations=30000))

        def state_after(fn):
            fn()
            st = np.random.get_state()
            return st[1].copy(), st[2]
        leg = _host_vs_device("the same ratio passed over", lambda: state_after(host), lambda: state_after(skip), repeats,
                              lambda a, b: np.array_equal(a[0], b[0]) and a[1] == b[1])
        legs.append(dict(leg, regions=r, permutations=30000))
    r = max(regions)
    ns = {s: argparse.Namespace(num_regions=r, num_samples_save=perms, sampler=s, device=dev) for s in ("host", "device")}
    leg = _host_vs_device("stage 1: all_orders", lambda: wide_stage.generate_all_orders(None, ns["host"], save=False),
                          lambda: wide_stage.generate_all_orders(None, ns["device"], save=False), repeats,
                          lambda a, b: a.dtype == b.dtype and np.array_equal(a, b))
    legs.append(dict(leg, regions=r, permutations=perms))
    return legs


def _write(path, res):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "wide_regions.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--perms", type=int, default=1000)
    ap.add_argument("--regions", type=int, nargs="+", default=[128, 256, 1024])
    ap.add_argument("--profile-step", type=int, default=0, metavar="R",
                    help="run one warmed step at R regions and exit (the program to put under rocprofv3 --kernel-trace --stats)")
    ap.add_argument("--route", choices=["keep", "prefix"], default="keep", help="the route of --profile-step")
    ap.add_argument("--prefix", action="store_true",
                    help="time wide.shapley, keep route against prefix route (leg 4), and put it under \"prefix\" in --out, keeping what is there")
    ap.add_argument("--interaction", action="store_true",
                    help="time the interaction stage only (legs 3a, 3b) and put it under \"interaction\" in --out, keeping what is there")
    ap.add_argument("--compact", action="store_true",
                    help="time wide.shapley of the other families, dense against compact coalitions (leg 5), and put it under "
                         "\"compact\" in --out, keeping what is there")
    ap.add_argument("--poses", action="store_true",
                    help="time a pose sweep, one wide.shapley per pose against wide.shapley_over_poses (leg 6), and put it under "
                         "\"poses\" in --out, keeping what is there")
    ap.add_argument("--sampler", action="store_true",
                    help="time the draws of a wide game, host against device (leg 7), and put it under \"sampler\" in --out, keeping what "
                         "is there")
    ap.add_argument("--profile-sampler", type=int, default=0, metavar="R",
                    help="run one warmed device draw of one ratio at R regions and exit (the program to put under rocprofv3 "
                         "--kernel-trace --stats)")
    ap.add_argument("--families", nargs="+", choices=COMPACT_FAMILIES, default=list(COMPACT_FAMILIES), help="the families of --compact")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_wide.py needs a GPU: a time taken elsewhere says nothing about the MI355X")
    dev = torch.device("cuda:0")
    if args.compact:
        res = json.load(open(args.out)) if os.path.exists(args.out) else {}
        legs = res.get("compact", {}).get("legs", [])
        for family in args.families:
            model = _family_model(family, dev)
            for r in (128, 1024):
                leg = compact_vs_dense(family, model, r, 5, dev)
                legs = [l for l in legs if (l["family"], l["regions"]) != (family, r)] + [leg]
            del model
            torch.cuda.empty_cache()
        res["compact"] = {"device": torch.cuda.get_device_name(0), "repeats": 5, "legs": legs}
        _write(args.out, res)
        return
    if args.sampler:
        res = json.load(open(args.out)) if os.path.exists(args.out) else {}
        res["sampler"] = dict(res.get("sampler", {}), device=torch.cuda.get_device_name(0), repeats=max(5, args.repeats),
                              legs=sampler_host_vs_device(max(5, args.repeats), dev))
        _write(args.out, res)
        return
    if args.profile_sampler:
        _, device, _ = _sampler_ratio(args.profile_sampler, dev)
        device()
        t, _ = _clock(device)
        print(json.dumps({"profile_sampler_regions": args.profile_sampler, "permutations": 30000, "runs": 2, "seconds_under_profiler": t}))
        return
    model = _model(dev)
    if args.profile_step:
        run, b = _wide_step(model, args.profile_step, args.perms, dev, args.route)
        run()
        t, _ = _clock(run)
        print(json.dumps({"profile_step_regions": args.profile_step, "route": args.route, "coalitions": b, "runs": 2,
                          "seconds_under_profiler": t}))
        return
    if args.prefix:
        from interpret_quality_amd import wide
        res = json.load(open(args.out)) if os.path.exists(args.out) else {}
        legs = [prefix_vs_keep(model, r, args.repeats, dev) for r in args.regions]
        res["prefix"] = {"device": torch.cuda.get_device_name(0), "repeats": max(5, args.repeats), "by_regions": legs,
                         "default_route_by_the_rule": "keep" if any(l["prefix_slower_beyond_spread"] for l in legs) else "prefix",
                         "default_route_in_this_build": wide.DEFAULT_ROUTE}
        _write(args.out, res)
        return
    if args.poses:
        res = json.load(open(args.out)) if os.path.exists(args.out) else {}
        legs = [poses_batched_vs_looped(model, r, dev) for r in (128, 1024)]
        res["poses"] = {"device": torch.cuda.get_device_name(0), "repeats": 5, "by_regions": legs,
                        "batching_stays_by_the_rule": not any(l["batched_slower_beyond_spread"] for l in legs)
                        and any(l["batched_faster"] for l in legs)}
        _write(args.out, res)
        return
    if args.interaction:
        res = json.load(open(args.out)) if os.path.exists(args.out) else {}
        res["interaction"] = {"device": torch.cuda.get_device_name(0), "repeats": args.repeats,
                              "wide": [interaction_rate(model, r, args.repeats, dev) for r in (128, 1024)],
                              "wide_vs_narrow": interaction_wide_vs_narrow(model, args.repeats, dev)}
        _write(args.out, res)
        return
    res = {"device": torch.cuda.get_device_name(0), "repeats": args.repeats,
           "wide_vs_narrow": [wide_vs_narrow(model, r, 1000, args.repeats, dev) for r in (32, 64)],
           "wide": [wide_rate(model, r, args.perms, args.repeats, dev) for r in args.regions]}
    _write(args.out, res)


if __name__ == "__main__":
    main()
