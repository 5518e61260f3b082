"""final_wide_shapley.py - stage 1 (shapley_stage.py, the mirror of final_shapley_value.py) for more than 64 regions, up to one
region per point (``--num_regions`` = the number of points: every point is a player).

Same artefacts, names and formats as stage 1, per selected cloud, under the experiment folder that ``exp_folder``
derives from ``--num_regions`` - so a run never overwrites a 32-region run:

    region_id.npy  norm_factor.npy  all_orders.npy  shapley/<i>_<count>.npy  region_shapley/<i>_<count>.npy  region_sv_all.npy

The permutations come from NumPy's global generator on the host, exactly as the reference's generate_all_orders draws them
(final_shapley_value.py:59-72); the device sampler of stage 1 stays a 64-region kernel.  The FPS centres go to their own
fps_<dataset>_<N>_<R>_index_final30.npy.  ``--route prefix|keep`` picks how ``wide.shapley`` evaluates the prefix coalitions (the
same bits either way), ``--coalitions dense|compact`` how a family other than PointNet evaluates them (wide.py).  Single process: under several ranks rank 0 does the work and the others wait.  The
multi-order interactions on these region ids: final_wide_interaction.py (wide_interaction_stage.py); the pose sweeps and the
smoothness stage on these region ids and permutations: final_wide_pose.py (wide_pose_stage.py) and final_wide_smoothness.py
(wide_smoothness_stage.py), sharded over the ranks.
"""
import numpy as np
import torch

from . import dist as iqdist
from . import hip_ops, wide
from . import shapley_stage as stage1
from .final_util import get_folder_name_list, load_model

DEFAULT_REGIONS = 128
MIN_REGIONS = 65          # up to 64 regions: final_shapley_value.py


def generate_all_orders(result_path, args, save=True):
    """final_shapley_value.py:59-72 as it stands: ``num_samples_save`` permutations of 0..R-1 from NumPy's GLOBAL generator."""
    rows = [np.random.permutation(np.arange(0, args.num_regions, 1)).reshape((1, -1)) for _ in range(args.num_samples_save)]
    all_orders = np.concatenate(rows, axis=0)
    if save:
        np.save(result_path + "all_orders.npy", all_orders)
    return all_orders


def cal_region_id(data, fps_index, result_path, save=True):
    """final_shapley_value.py:20-35 for up to wide.MAX_REGIONS centres.  data (1,N,3), fps_index (R,) -> (N,) int64 ndarray."""
    idx = hip_ops.as_i32(fps_index, data.device)
    region_id = hip_ops.region_assign_wide(data[0].contiguous(), idx).cpu().numpy().astype(np.int64)
    if save:
        np.save(result_path + "region_id.npy", region_id)
    return region_id


def run(args):
    model = load_model(args)
    with torch.no_grad():
        for i, name, result_path, data, lbl, fps_index in stage1.selected_clouds(args, get_folder_name_list(args), generate_all_orders):
            region_id = cal_region_id(data, fps_index, result_path)
            center = torch.mean(data, dim=1).squeeze()
            stage1.cal_norm_factor(model, data, lbl, center, result_path, args)
            all_orders = generate_all_orders(result_path, args)
            print("pointcloud:%s, index:%d, regions:%d, samples:%d" % (name, i, args.num_regions, len(all_orders)))
            snaps, region_sv_all, _ = wide.shapley(model, data, lbl, region_id, all_orders, args, snap_counts=stage1.SAMPLE_NUMS,
                                                   route=args.route, coalitions=getattr(args, "coalitions", None))
            for count, running in snaps.items():
                stage1.save_shapley(running, i, count, result_path, region_id, args)
            np.save(result_path + "region_sv_all.npy", region_sv_all)


def make_args(argv=None):
    parser = stage1.build_parser()
    parser.add_argument("--route", choices=wide.ROUTES, default=None,
                        help="how the prefix coalitions are evaluated: prefix = straight from the permutations (PointNet), keep = "
                             "through keep rows; the same bits either way (default: prefix where the model has it)")
    parser.add_argument("--coalitions", choices=wide.COALITIONS, default=None,
                        help="how a family other than PointNet evaluates the coalitions: dense = its dense forward on materialised "
                             "clouds (the default), compact = its compact coalition path; the same artefacts, equal to rounding")
    return stage1.parse_game_args(parser, argv, DEFAULT_REGIONS, MIN_REGIONS, wide.MAX_REGIONS,
                                  "the wide stage takes %d .. %d regions (final_shapley_value.py: up to 64)" % (MIN_REGIONS, wide.MAX_REGIONS))


@iqdist.record
def main(argv=None):
    args = make_args(argv)
    stage1.finish_args(args)
    if args.num_regions > args.num_points:
        raise SystemExit("--num_regions %d exceeds the %d points of a cloud" % (args.num_regions, args.num_points))
    stage1.rank0_only(run, args, "wide")


if __name__ == "__main__":
    main()
