#!/usr/bin/env python3
"""Rate of the PointNet coalition chain kernels by item size, and what the launch order does with it.
One process, HIP-event times of the two chain launches (profiler slots 1 and 2) around model.coalition_logits on the synthetic cloud.

  homogeneous batches: random subsets of exactly k regions - a k-region item beside nothing but its like ("short beside short");
  two mixed batches of the same items: half full sets, half one-region sets, in plain LPT order (all long, then all short) and with
  the short items dealt out among the long ones, and the difference against what the homogeneous figures predict.  The mixed
  order is an experiment that was not adopted: this part runs only on a library built with tools/experiments/chain_mixed_order.patch
  (there the mixed order is the default and tuning key 5 = 60 is plain LPT); the product library prints the LPT figure alone.
  On the product library every batch runs under tuning key 5 = 60, which there means: compute every repeated full or empty set - a
  batch of nothing but full sets would otherwise be one item and 8191 copies.

usage: python tools/chain_by_size.py [--batch 8192] [--regions 32] [--repeats 3] [--out FILE]"""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from interpret_quality_amd import _lib, hip_ops, synth, tuning  # noqa: E402
from interpret_quality_amd.pointnet import PointNetCls  # noqa: E402

KS = (0, 1, 2, 3, 5, 8, 12, 16, 24, 32)
NO_DEDUP_TWIN = "chain_no_dedup"      # 5 = 60, the product library: every repeated set computed
LPT_TWIN = NO_DEDUP_TWIN              # the patched library gives the same value another meaning: plain LPT

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=8192)
ap.add_argument("--regions", type=int, default=32)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--out", default=None, help="also write the report here")
args = ap.parse_args()

lib = _lib.load()
PATCHED = hasattr(lib, "iq_debug_chain_order")      # the host twin only the experiment patch exports
BASE = None if PATCHED else NO_DEDUP_TWIN
dev = torch.device("cuda:0")
model = PointNetCls(None)
model.load_state_dict(synth.to_torch(synth.pointnet_state_dict(0)))
model = model.to(dev).eval()
pts, _ = synth.make_cloud(0)
data = torch.from_numpy(pts).unsqueeze(0).to(dev)
N, R, B = data.shape[1], args.regions, args.batch
region_id = hip_ops.region_assign(data[0].contiguous(), hip_ops.fps(data, R)[0].contiguous()).reshape(1, -1)
center = torch.mean(data, dim=1).contiguous()
sizes = np.bincount(region_id.cpu().numpy().reshape(-1), minlength=R).astype(np.int64)
rng = np.random.default_rng(0)
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def finish():
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    sys.exit(0)


def subsets(k, b):
    """(b,) uint64 masks of exactly k regions each, drawn at random."""
    bits = np.argsort(rng.random((b, R)), axis=1) < k
    return (bits.astype(np.uint64) << np.arange(R, dtype=np.uint64)).sum(axis=1, dtype=np.uint64)


def tiles_of(masks):
    """Executed 32-row tiles of a batch: each coalition's distinct rows (kept points + the centre row when anything is masked)."""
    bits = ((masks[:, None] >> np.arange(R, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(np.int64)
    kept = bits @ sizes
    rows = kept + (kept < N)
    return int(((rows + 31) // 32).sum())


def read(slot):
    ms, n, work = ctypes.c_double(0), ctypes.c_int(0), ctypes.c_double(0)
    _lib.check(lib.iq_profile_read_work(slot, ctypes.byref(ms), ctypes.byref(n), ctypes.byref(work)), "iq_profile_read_work")
    return ms.value * 1e3 / max(n.value, 1)


def launch_us(masks, twin=BASE):
    """us per chain launch (mean of the feature-STN and the trunk launch), one figure per repeat after one untimed call."""
    keep = hip_ops.masks_to_tensor(masks, dev)
    out = []
    with tuning.twin(twin):
        for rep in range(args.repeats + 1):
            lib.iq_profile_enable(1)
            model.coalition_logits(data, center, region_id, keep, None, num_regions=R, validate=False)
            torch.cuda.synchronize()
            lib.iq_profile_enable(0)
            f, t = read(1), read(2)
            read(0), read(3)
            if rep:
                out.append(0.5 * (f + t))
    return np.array(out)


def fmt(a):
    return "%9.1f  [%s]  spread %.1f %%" % (np.median(a), " ".join("%.1f" % x for x in a), 100.0 * (a.max() - a.min()) / np.median(a))


say("# python tools/chain_by_size.py " + " ".join(sys.argv[1:]))
say("# %s; N = %d points, R = %d regions of %d..%d points, batches of %d coalitions, %d repeats after one untimed call"
    % (torch.cuda.get_device_name(0), N, R, sizes.min(), sizes.max(), B, args.repeats))
say("# us per launch = mean of the two chain launches (feature STN, trunk) of a call; tiles = executed 32-row tiles of one launch")
say("#  k   tiles/launch  tiles/item   us per launch: median [repeats] spread        ns per tile   x of k = %d" % KS[-1])
homog = {}
for k in KS:
    masks = subsets(k, B)
    homog[k] = (launch_us(masks), tiles_of(masks))
ref = np.median(homog[KS[-1]][0]) * 1e3 / homog[KS[-1]][1]
for k in KS:
    us, tiles = homog[k]
    ns = np.median(us) * 1e3 / tiles
    say("%4d  %12d  %10.2f  %s   %10.2f   %6.2f" % (k, tiles, tiles / B, fmt(us), ns, ns / ref))
worst = max(np.median(homog[k][0]) * 1e3 / homog[k][1] / ref for k in KS if k <= 5)
say("# decision rule: the homogeneous batches with k <= 5 take up to %.2f x the ns per tile of k = %d (the premise holds above 1.10)"
    % (worst, KS[-1]))

say()
say("# mixed batch: %d full sets and %d one-region sets, the same items in both orders" % (B // 2, B - B // 2))
masks = np.concatenate([subsets(R, B // 2), subsets(1, B - B // 2)])
masks = masks[rng.permutation(B)]
t_long, t_short = tiles_of(masks[masks == masks.max()]), tiles_of(masks[masks != masks.max()])
if not PATCHED:      # the product library: no mixed order
    say("plain LPT (the library's order)   %s" % fmt(launch_us(masks)))
    say("# mixed order: not in this library (tools/experiments/chain_mixed_order.patch)")
    finish()
lpt, mixed = launch_us(masks, LPT_TWIN), launch_us(masks, None)
lpt2 = launch_us(masks, LPT_TWIN)
say("plain LPT (key 5 = %d)   %s" % (tuning.TWINS[LPT_TWIN], fmt(lpt)))
say("mixed order (default)   %s" % fmt(mixed))
say("plain LPT once more     %s" % fmt(lpt2))
d = np.median(np.concatenate([lpt, lpt2])) - np.median(mixed)
ns_long, ns_short = ref, np.median(homog[1][0]) * 1e3 / homog[1][1]
say("# LPT - mixed: %.1f us per launch (%.2f %% of the LPT launch)" % (d, 100.0 * d / np.median(np.concatenate([lpt, lpt2]))))
say("# predicted from the homogeneous figures: LPT = %d long tiles x %.2f ns + %d short tiles x %.2f ns = %.1f us; every tile at the"
    % (t_long, ns_long, t_short, ns_short, (t_long * ns_long + t_short * ns_short) * 1e-3))
say("# long rate = %.1f us; the most a launch order can give back = %.1f us" % ((t_long + t_short) * ns_long * 1e-3, t_short * (ns_short - ns_long) * 1e-3))
finish()
