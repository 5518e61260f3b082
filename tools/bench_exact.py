#!/usr/bin/env python3
"""Times the lattice reductions of csrc/iq_lattice.hip (not the flagship workload: that is bench.py).

    python tools/bench_exact.py [--out profiles/exact_lattice.json] [--sizes 16 20 24] [--no-model]

For n = 16, 20, 24 players and all n(n-1)/2 pairs, on a seeded random table: the time of each reduction (device events around
``reps`` back-to-back calls after a warm-up, scratch allocated outside the window), the bytes it must move at least (the table
once per player for the Shapley values, once per pair for the interactions, the table in and the float64 dividends out for the
Moebius transform), the resulting rate, and - the yardstick, timed in the same run - a plain device-to-device copy of the same
table.  Then, for PointNet at n = 20, the share of the three reductions in a whole exact run (value table + reductions)."""
import argparse
import ctypes
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from interpret_quality_amd import _lib, exact, hip_ops, synth  # noqa: E402


def _timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3 / reps


def lattice_times(n, dev, reps):
    lib = _lib.load()
    v = torch.from_numpy((np.random.default_rng(n).standard_normal(1 << n) * 3).astype(np.float32)).to(dev)
    pairs = hip_ops.as_i32(hip_ops.all_pairs(n), dev)
    p = pairs.shape[0]
    scratch = torch.empty((lib.iq_exact_scratch_bytes(n, p) // 8,), dtype=torch.float64, device=dev)
    phi = torch.empty((n,), dtype=torch.float64, device=dev)
    inter = torch.empty((p, n - 1), dtype=torch.float64, device=dev)
    a = torch.empty((1 << n,), dtype=torch.float64, device=dev)
    dst = torch.empty_like(v)
    ptr, st = (lambda t: ctypes.c_void_p(t.data_ptr())), (lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    table = 4 << n
    calls = {
        "shapley": (lambda: _lib.check(lib.iq_exact_shapley(ptr(v), n, ptr(phi), ptr(scratch), scratch.numel() * 8, st()), "shapley"), n * table),
        "interactions": (lambda: _lib.check(lib.iq_exact_interactions(ptr(v), n, ptr(pairs), p, ptr(inter), ptr(scratch), scratch.numel() * 8, st()),
                                            "interactions"), p * table),
        "moebius": (lambda: _lib.check(lib.iq_moebius(ptr(v), n, ptr(a), st()), "moebius"), 3 * table),
        "copy_d2d": (lambda: dst.copy_(v), 2 * table),
    }
    out = {"n": n, "pairs": p, "table_bytes": table}
    for name, (fn, nbytes) in calls.items():
        t = _timed(fn, reps)
        out[name] = {"seconds": t, "min_bytes": nbytes, "GB_per_s": nbytes / t / 1e9}
    return out


def pointnet_share(n, dev):
    """A whole exact run of PointNet with n regions: value table (2^n coalitions), then the three reductions."""
    from types import SimpleNamespace
    from interpret_quality_amd.pointnet import PointNetCls
    model = PointNetCls(None)
    model.load_state_dict(synth.to_torch(synth.pointnet_state_dict(0)))
    model = model.to(dev).eval()
    pts, label = synth.make_cloud(0)
    data, lbl = torch.from_numpy(pts).unsqueeze(0).to(dev), torch.tensor([label], device=dev)
    rid = hip_ops.region_assign(data[0].contiguous(), hip_ops.fps(data, n)[0].contiguous()).cpu().numpy().astype(np.int64)
    args = SimpleNamespace(model="pointnet", softmax_type="modified", num_points=1024, num_regions=n, verbose=False)
    exact.value_table(model, data, lbl, rid, args, players=list(range(min(n, 10))))       # warm-up: engine, workspace, code objects
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    v = exact.value_table(model, data, lbl, rid, args)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    phi, inter, a = hip_ops.exact_shapley(v), hip_ops.exact_interactions(v), hip_ops.moebius(v)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    return {"n": n, "coalitions": 1 << n, "value_table_seconds": t1 - t0, "coalitions_per_s": (1 << n) / (t1 - t0),
            "reductions_seconds": t2 - t1, "reductions_share": (t2 - t1) / (t2 - t0), "sum_phi": float(phi.sum()),
            "v_full_minus_v_empty": float(v[-1] - v[0])}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "exact_lattice.json"))
    ap.add_argument("--sizes", type=int, nargs="+", default=[16, 20, 24])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--model_n", type=int, default=20)
    ap.add_argument("--no-model", action="store_true")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_exact.py needs a GPU: a time taken elsewhere says nothing about the MI355X")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "lattice": [lattice_times(n, dev, args.reps) for n in args.sizes]}
    if not args.no_model:
        res["pointnet_exact_run"] = pointnet_share(args.model_n, dev)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
