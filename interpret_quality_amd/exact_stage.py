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

import numpy as np
import torch

from . import dist as iqdist
from . import exact, hip_ops
from . import shapley_stage as stage1
from .final_util import get_folder_name_list, load_model, mkdir

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
    with torch.no_grad():
        # a cloud that is not selected still draws stage 1's permutations: the stream runs on from cloud to cloud
        for i, name, result_path, data, lbl, fps_index in stage1.selected_clouds(args, get_folder_name_list(args), stage1.generate_all_orders):
            mkdir(result_path + "exact/")
            region_id = stage1.cal_region_id(data, fps_index, result_path, save=False)
            all_orders = stage1.generate_all_orders(result_path, args, save=False)
            out = exact_one_cloud(model, data, lbl, region_id, all_orders, args)
            for key in ("value_table", "region_shapley_value", "interaction_all_orders"):
                np.save(result_path + "exact/%s.npy" % key, out[key])
            with open(result_path + "exact/sampling_error.json", "w") as f:
                json.dump({"num_regions": args.num_regions, "sample_counts": out["sampling_error"]}, f, indent=1)
            last = out["sampling_error"][-1] if out["sampling_error"] else None
            print("pointcloud:%s, index:%d, coalitions:%d, sum(phi)=%.6f%s" % (
                name, i, 1 << args.num_regions, out["region_shapley_value"].sum(),
                ", %d samples: rms error %.4g (%.2f standard errors)" % (last["samples"], last["rms_error"], last["rms_error_in_se"])
                if last else ""))


def make_args(argv=None):
    parser = stage1.build_parser()
    parser.add_argument("--chunk", type=int, default=1 << 16, help="coalitions evaluated per step of the enumeration")
    return stage1.parse_game_args(parser, argv, DEFAULT_REGIONS, 1, exact.MAX_PLAYERS,
                                  "an exact game enumerates 2^num_regions coalitions; at most %d regions are supported "
                                  "(the sampling stage final_shapley_value.py has no such limit)" % exact.MAX_PLAYERS)


@iqdist.record
def main(argv=None):
    args = make_args(argv)
    stage1.finish_args(args)
    stage1.rank0_only(run, args, "exact")


if __name__ == "__main__":
    main()
