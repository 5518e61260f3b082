"""final_wide_shapley.py - stage 1 (shapley_stage.py, the mirror of final_shapley_value.py) for more than 64 regions, up to one
region per point (``--num_regions`` = the number of points: every point is a player).

Same artefacts, names and formats as stage 1, per selected cloud, under the experiment folder that ``exp_folder``
derives from ``--num_regions`` - so a run never overwrites a 32-region run:

    region_id.npy  norm_factor.npy  all_orders.npy  shapley/<i>_<count>.npy  region_shapley/<i>_<count>.npy  region_sv_all.npy

The permutations come from NumPy's global generator on the host, exactly as the reference's generate_all_orders draws them
(final_shapley_value.py:59-72); the device sampler of stage 1 stays a 64-region kernel.  The FPS centres go to their own
fps_<dataset>_<N>_<R>_index_final30.npy.  Single process: under several ranks rank 0 does the work and the others wait.  The
multi-order interactions on these region ids: final_wide_interaction.py (wide_interaction_stage.py).  The smoothness and pose
stages have no wide form.
"""
import os

import numpy as np
import torch

from . import dist as iqdist
from . import hip_ops, wide
from . import shapley_stage as stage1
from .final_util import NUM_SAMPLES_SAVE, get_folder_name_list, load_model, mkdir

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
                generate_all_orders(result_path, args, save=False)   # the stream runs on from cloud to cloud: draw, do not compute
                continue
            mkdir(result_path)
            data, lbl = data.to(args.device), lbl.to(args.device)
            region_id = cal_region_id(data, fps_indices[i], result_path)
            center = torch.mean(data, dim=1).squeeze()
            stage1.cal_norm_factor(model, data, lbl, center, result_path, args)
            all_orders = generate_all_orders(result_path, args)
            print("pointcloud:%s, index:%d, regions:%d, samples:%d" % (folder_name_list[i], i, args.num_regions, len(all_orders)))
            snaps, region_sv_all, _ = wide.shapley(model, data, lbl, region_id, all_orders, args, snap_counts=stage1.SAMPLE_NUMS)
            for count, running in snaps.items():
                stage1.save_shapley(running, i, count, result_path, region_id, args)
            np.save(result_path + "region_sv_all.npy", region_sv_all)


def make_args(argv=None):
    parser = stage1.build_parser()
    parser.add_argument("--num_samples_save", type=int, default=NUM_SAMPLES_SAVE)   # additive, as in stage 1
    parser.add_argument("--num_regions", type=int, default=DEFAULT_REGIONS)         # additive
    args = parser.parse_args(argv)
    if not MIN_REGIONS <= args.num_regions <= wide.MAX_REGIONS:
        parser.error("--num_regions %d: the wide stage takes %d .. %d regions (final_shapley_value.py: up to 64)"
                     % (args.num_regions, MIN_REGIONS, wide.MAX_REGIONS))
    return args


@iqdist.record
def main(argv=None):
    args = make_args(argv)
    stage1.finish_args(args)
    if args.num_regions > args.num_points:
        raise SystemExit("--num_regions %d exceeds the %d points of a cloud" % (args.num_regions, args.num_points))
    if iqdist.rank() == 0:
        run(args)
    else:
        print("rank %d: the wide stage runs on rank 0 only; waiting" % iqdist.rank())
    iqdist.barrier()


if __name__ == "__main__":
    main()
