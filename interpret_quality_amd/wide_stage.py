"""final_wide_shapley.py - stage 1 (shapley_stage.py, the mirror of final_shapley_value.py) for more than 64 regions, up to one
region per point (``--num_regions`` = the number of points: every point is a player).

Same artefacts, names and formats as stage 1, per selected cloud, under the experiment folder that ``exp_folder``
derives from ``--num_regions`` - so a run never overwrites a 32-region run:

    region_id.npy  norm_factor.npy  all_orders.npy  shapley/<i>_<count>.npy  region_shapley/<i>_<count>.npy  region_sv_all.npy

The permutations come from NumPy's global generator, exactly as the reference's generate_all_orders draws them
(final_shapley_value.py:59-72): on the host, or with ``--sampler device`` the same stream continued on the GPU (stage 1's device
sampler in its wide form, iq_sample_permutations_wide; the same all_orders.npy byte for byte).  The FPS centres go to their own
fps_<dataset>_<N>_<R>_index_final30.npy.  ``--route prefix|keep`` picks how ``wide.shapley`` evaluates the prefix coalitions (the
same bits either way), ``--coalitions dense|compact`` how a family other than PointNet evaluates them (wide.py).  Single process: under several ranks rank 0 does the work and the others wait.  The
multi-order interactions on these region ids: final_wide_interaction.py (wide_interaction_stage.py); the pose sweeps and the
smoothness stage on these region ids and permutations: final_wide_pose.py (wide_pose_stage.py) and final_wide_smoothness.py
(wide_smoothness_stage.py), sharded over the ranks.

What the four wide stages share lives here too: the --route / --coalitions / --num_samples / --sampler flags, the region-count message, the
checks after finish_args, the "not found: run ... first" check of an earlier stage's files, and ``GAME`` - the wide game that the
pose and smoothness stages pass to pose_sweep's and smoothness's per-cloud loops.
"""
import os

import numpy as np
import torch

from . import dist as iqdist
from . import hip_ops, pose_sweep, wide
from . import shapley_stage as stage1
from .final_util import NUM_SAMPLES, get_folder_name_list, load_model

DEFAULT_REGIONS = 128
MIN_REGIONS = 65          # up to 64 regions: final_shapley_value.py


# ---- what the four wide stages share: flags, checks, stage 1's files -------------------------------
SAMPLERS = ("host", "device")


def add_wide_flags(parser, route=True, num_samples=False):
    """--coalitions and --sampler, and where the stage has them --route and --num_samples."""
    parser.add_argument("--sampler", choices=SAMPLERS, default="host",
                        help="where final_wide_shapley.py draws the permutations and final_wide_interaction.py the sampled contexts: host = "
                             "NumPy's global generator, device = the same stream continued on the GPU (iq_sample_permutations_wide); the "
                             "same artefacts, byte for byte.  The stages that draw nothing take the flag and ignore it (scripts/exp_wide.sh "
                             "passes one EXTRA to all of them)")
    if route:
        parser.add_argument("--route", choices=wide.ROUTES, default=None,
                            help="how the prefix coalitions are evaluated: prefix = straight from the permutations (PointNet), keep = "
                                 "through keep rows; the same bits either way (default: prefix where the model has it)")
    parser.add_argument("--coalitions", choices=wide.COALITIONS, default=None,
                        help="how a family other than PointNet evaluates the coalitions: dense = its dense forward on materialised "
                             "clouds (the default), compact = its compact coalition path; the same artefacts, equal to rounding")
    if num_samples:
        parser.add_argument("--num_samples", type=int, default=NUM_SAMPLES,
                            help="permutations per pose: the first rows of the all_orders.npy that final_wide_shapley.py wrote")


def parse_wide_args(parser, argv, narrow_scripts, samples=True):
    """shapley_stage.parse_game_args for MIN_REGIONS .. wide.MAX_REGIONS regions; ``narrow_scripts``: where fewer regions go."""
    return stage1.parse_game_args(parser, argv, DEFAULT_REGIONS, MIN_REGIONS, wide.MAX_REGIONS,
                                  "the wide stage takes %d .. %d regions (%s: up to 64)" % (MIN_REGIONS, wide.MAX_REGIONS, narrow_scripts),
                                  samples=samples)


def check_points(args):
    """What every wide stage refuses after finish_args: more regions than points."""
    if args.num_regions > args.num_points:
        raise SystemExit("--num_regions %d exceeds the %d points of a cloud" % (args.num_regions, args.num_points))


def check_wide_args(args):
    """``check_points``, and for the stages with --num_samples: fewer than one permutation."""
    check_points(args)
    if args.num_samples < 1:
        raise SystemExit("--num_samples %d: at least one permutation" % args.num_samples)


def require(path, args, first="final_wide_shapley.py"):
    """SystemExit naming the stage that writes ``path`` when it is not there."""
    if not os.path.exists(path):
        raise SystemExit("%s not found: run %s --num_regions %d first" % (path, first, args.num_regions))


def selected_folders(args, names):
    """pose_sweep.selected_folders; SystemExit (``require``) when stage 1 has not written a cloud's region ids or permutations."""
    out = pose_sweep.selected_folders(args, names)
    for _, base in out:
        for f in ("region_id.npy", "all_orders.npy"):
            require(base + f, args)
    return out


def load_orders(base_folder, args):
    """The first ``--num_samples`` rows of the cloud's all_orders.npy; more than the file holds is an error."""
    orders = np.load(base_folder + "all_orders.npy")
    if args.num_samples > orders.shape[0]:
        raise SystemExit("--num_samples %d exceeds the %d permutations of %sall_orders.npy (final_wide_shapley.py "
                         "--num_samples_save)" % (args.num_samples, orders.shape[0], base_folder))
    return orders[:args.num_samples]


def sharded_shapley(model, data, poses, lbl, region_id, orders, args):
    """wide.sharded_shapley as the per-cloud loops call it: route and coalitions from the flags, and no logits."""
    return wide.sharded_shapley(model, data, poses, lbl, region_id, orders, args, route=args.route, coalitions=args.coalitions) + (None,)


GAME = pose_sweep.Game(selected_folders, load_orders, sharded_shapley)   # the wide game of the pose and smoothness stages


def _device_orders(args, skip=False):
    """``num_samples_save`` permutations from NumPy's GLOBAL generator, continued on the device and handed back (one sync)."""
    state = hip_ops.mt_state_to_device(args.device)
    orders = hip_ops.sample_permutations_wide(state, args.num_samples_save, args.num_regions, skip=skip)
    hip_ops.mt_state_to_host(state, set_global=True)
    return None if skip else orders.cpu().numpy().astype(np.int64)


def skip_all_orders(result_path, args, save=False):
    """What ``generate_all_orders`` draws, drawn and dropped: the permutations of a cloud that is not selected.  With
    ``--sampler device`` the device sampler's skip mode: nothing is written anywhere."""
    if getattr(args, "sampler", "host") == "device":
        _device_orders(args, skip=True)
    else:
        generate_all_orders(result_path, args, save=False)


def generate_all_orders(result_path, args, save=True):
    """final_shapley_value.py:59-72 as it stands: ``num_samples_save`` permutations of 0..R-1 from NumPy's GLOBAL generator - on the
    host, or with ``--sampler device`` the same stream on the device (the same int64 array, the same generator state afterwards)."""
    if getattr(args, "sampler", "host") == "device":
        all_orders = _device_orders(args)
    else:
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
        for i, name, result_path, data, lbl, fps_index in stage1.selected_clouds(args, get_folder_name_list(args), skip_all_orders):
            region_id = cal_region_id(data, fps_index, result_path)
            center = torch.mean(data, dim=1).squeeze()
            stage1.cal_norm_factor(model, data, lbl, center, result_path, args)
            all_orders = generate_all_orders(result_path, args)
            print("pointcloud:%s, index:%d, regions:%d, samples:%d" % (name, i, args.num_regions, len(all_orders)))
            snaps, region_sv_all, _ = wide.shapley(model, data, lbl, region_id, all_orders, args, snap_counts=stage1.SAMPLE_NUMS,
                                                   route=args.route, coalitions=args.coalitions)
            for count, running in snaps.items():
                stage1.save_shapley(running, i, count, result_path, region_id, args)
            np.save(result_path + "region_sv_all.npy", region_sv_all)


def make_args(argv=None):
    parser = stage1.build_parser()
    add_wide_flags(parser)
    return parse_wide_args(parser, argv, "final_shapley_value.py")


@iqdist.record
def main(argv=None):
    args = make_args(argv)
    stage1.finish_args(args)
    check_points(args)
    stage1.rank0_only(run, args, "wide")


if __name__ == "__main__":
    main()
