"""final_exact_shapley.py - the exact counterpart of stage 1 (shapley_stage.py; the reference has none: it only samples).

Per selected cloud, under the experiment folder that ``exp_folder`` derives from ``--num_regions`` (default 16 here: 65 536
coalitions; refused above 24):

    exact/value_table.npy             (2^n,) float32   reward of every coalition, bit k of the index = region k kept
    exact/region_shapley_value.npy    (n,) float64     the exact Shapley values
    exact/interaction_all_orders.npy  (n(n-1)/2, n-1) float64   I_ij^(m) over ALL contexts, pairs in lexicographic order
    exact/sampling_error.json         how far stage 1's running estimate (its sample counts 100 .. 1000, the permutations stage 1
                                      would draw for the same seed) is from the exact values: max and RMS over the regions, in
                                      reward units and in units of the estimate's standard error

The sampled estimate is read off the value table (a prefix coalition's reward is a table entry), not run through the network
again.  Single process: under several ranks rank 0 does the work and the others wait at the end.
"""
import json
import os

import numpy as np
import torch

from . import dist as iqdist
from . import exact, hip_ops
from . import shapley_stage as stage1
from .final_util import NUM_SAMPLES_SAVE, get_folder_name_list, load_model, mkdir

DEFAULT_REGIONS = 16


def exact_one_cloud(model, data, lbl, region_id, all_orders, args):
    """-> dict of the four artefacts of one cloud (ndarrays and the sampling-error list)."""
    v = exact.value_table(model, data, lbl, region_id, args, chunk=args.chunk)
    phi, _, _ = exact.shapley(model, data, lbl, region_id, args, v=v)
    inter = exact.interactions(model, data, lbl, region_id, args, v=v)
    snaps, rows = exact.sampled_from_table(v, all_orders, stage1.SAMPLE_NUMS)
    return {"value_table": v.cpu().numpy(), "region_shapley_value": phi, "interaction_all_orders": inter,
            "sampling_error": exact.sampling_error(phi, snaps, rows)}


def run(args):
    model = load_model(args)
    folder_name_list = get_folder_name_list(args)
    if not os.path.exists(stage1.fps_index_path(args)):
        stage1.save_fps(args)
    fps_indices = np.load(stage1.fps_index_path(args))
    subset = getattr(args, "cloud_subset", None)
    with torch.no_grad():
        for i, (data, lbl) in enumerate(stage1.data_loader(args)):
            if subset is not None and i > max(subset):
                break
            result_path = args.exp_folder + "%s/" % folder_name_list[i]
            if not iqdist.cloud_selected(args, i):
                stage1.generate_all_orders(result_path, args, save=False)   # keep stage 1's permutation stream per cloud
                continue
            mkdir(result_path + "exact/")
            data, lbl = data.to(args.device), lbl.to(args.device)
            region_id = stage1.cal_region_id(data, fps_indices[i], result_path, save=False)
            all_orders = stage1.generate_all_orders(result_path, args, save=False)
            out = exact_one_cloud(model, data, lbl, region_id, all_orders, args)
            for name in ("value_table", "region_shapley_value", "interaction_all_orders"):
                np.save(result_path + "exact/%s.npy" % name, out[name])
            with open(result_path + "exact/sampling_error.json", "w") as f:
                json.dump({"num_regions": args.num_regions, "sample_counts": out["sampling_error"]}, f, indent=1)
            last = out["sampling_error"][-1] if out["sampling_error"] else None
            print("pointcloud:%s, index:%d, coalitions:%d, sum(phi)=%.6f%s" % (
                folder_name_list[i], i, 1 << args.num_regions, out["region_shapley_value"].sum(),
                ", %d samples: rms error %.4g (%.2f standard errors)" % (last["samples"], last["rms_error"], last["rms_error_in_se"])
                if last else ""))


def make_args(argv=None):
    parser = stage1.build_parser()
    parser.add_argument("--num_samples_save", type=int, default=NUM_SAMPLES_SAVE)   # additive, as in stage 1
    parser.add_argument("--num_regions", type=int, default=DEFAULT_REGIONS)          # additive
    parser.add_argument("--chunk", type=int, default=1 << 16, help="coalitions evaluated per step of the enumeration")
    args = parser.parse_args(argv)
    if not 1 <= args.num_regions <= exact.MAX_PLAYERS:
        parser.error("--num_regions %d: an exact game enumerates 2^num_regions coalitions; at most %d regions are supported "
                     "(the sampling stage final_shapley_value.py has no such limit)" % (args.num_regions, exact.MAX_PLAYERS))
    return args


@iqdist.record
def main(argv=None):
    args = make_args(argv)
    stage1.finish_args(args)
    if iqdist.rank() == 0:
        run(args)
    else:
        print("rank %d: the exact stage runs on rank 0 only; waiting" % iqdist.rank())
    iqdist.barrier()


if __name__ == "__main__":
    main()
