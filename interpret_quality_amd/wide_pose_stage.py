"""final_wide_pose.py --mode trans|rotate|scale - stages 2-4 (pose_sweep.py, the mirror of final_{trans,rotate,scale}_center_enum_all.py)
for more than 64 regions, up to one region per point: region Shapley values of every selected cloud under 216 translations / 216
rotations / 30 scales, on the region ids and the first ``--num_samples`` permutations that final_wide_shapley.py wrote for the same
``--num_regions``.

Grids, perturbations and the log / save helpers are pose_sweep's own; the per-cloud loop is pose_sweep.test with the Shapley call
exchanged for ``wide.sharded_shapley`` - the poses (and the original cloud as pose 0) sharded over the ranks, one gather per
cloud, rank 0 writes.  Every pose goes through the existing wide coalition entries (wide.py); there is no second evaluation path.
Artefacts per selected cloud under ``<exp_folder of R>/<cloud>/<mode>_all/``:

    orig_shapley_value.npy (R,)   region_shapley_value.npy (P,R) float64   trans_vector.npy + trans_distance.npy | angle_tuple.npy |
    scale.npy   log.txt

The one deviation from the narrow stage: no ``all_logits.pt``.  It is (P, S(R+1), C) - 0.45 GB per sweep at R = 128 and 3.5 GB at
R = 1024 with 100 permutations - and nothing downstream reads it (final_gen_pair.py and final_result.py read
region_shapley_value.npy and the parameter files only).
"""
import os
import time

import numpy as np
import torch

from . import dist as iqdist
from . import pose_sweep, wide
from . import shapley_stage as stage1
from .final_util import NUM_SAMPLES, IOStream, get_folder_name_list, load_model, mkdir
from .wide_stage import DEFAULT_REGIONS, MIN_REGIONS

MODES = {"trans": (pose_sweep.generate_trans_vector, pose_sweep.translate_pc, pose_sweep.print_trans_info, pose_sweep.save_trans_info),
         "rotate": (pose_sweep.generate_rotate_angle, pose_sweep.rotate_xyz, pose_sweep.print_rotate_info, pose_sweep.save_rotate_info),
         "scale": (pose_sweep.generate_scale, pose_sweep.scale_pc, pose_sweep.print_scale_info, pose_sweep.save_scale_info)}


def add_wide_flags(parser):
    """--route, --coalitions (wide_stage.py) and --num_samples: the flags the wide pose and smoothness stages share."""
    parser.add_argument("--route", choices=wide.ROUTES, default=None,
                        help="how the prefix coalitions are evaluated: prefix = straight from the permutations (PointNet), keep = "
                             "through keep rows; the same bits either way (default: prefix where the model has it)")
    parser.add_argument("--coalitions", choices=wide.COALITIONS, default=None,
                        help="how a family other than PointNet evaluates the coalitions: dense = its dense forward on materialised "
                             "clouds (the default), compact = its compact coalition path; the same artefacts, equal to rounding")
    parser.add_argument("--num_samples", type=int, default=NUM_SAMPLES,
                        help="permutations per pose: the first rows of the all_orders.npy that final_wide_shapley.py wrote")


def check_wide_args(args):
    """What both stages refuse after finish_args: more regions than points, fewer than one permutation."""
    if args.num_regions > args.num_points:
        raise SystemExit("--num_regions %d exceeds the %d points of a cloud" % (args.num_regions, args.num_points))
    if args.num_samples < 1:
        raise SystemExit("--num_samples %d: at least one permutation" % args.num_samples)


def selected_folders(args, names):
    """(index, base folder) of the clouds this call computes; SystemExit (wide_interaction_stage.run's message) when stage 1 has
    not written a cloud's region ids or permutations."""
    out = [(i, args.exp_folder + "%s/" % name) for i, name in enumerate(names) if iqdist.cloud_selected(args, i)]
    for _, base in out:
        for f in ("region_id.npy", "all_orders.npy"):
            if not os.path.exists(base + f):
                raise SystemExit("%s not found: run final_wide_shapley.py --num_regions %d first" % (base + f, args.num_regions))
    return out


def load_orders(base_folder, args):
    """The first ``--num_samples`` rows of the cloud's all_orders.npy; more than the file holds is an error."""
    orders = np.load(base_folder + "all_orders.npy")
    if args.num_samples > orders.shape[0]:
        raise SystemExit("--num_samples %d exceeds the %d permutations of %sall_orders.npy (final_wide_shapley.py "
                         "--num_samples_save)" % (args.num_samples, orders.shape[0], base_folder))
    return orders[:args.num_samples]


def test(args, get_transform_params_fn, disturb_fn, print_info_fn, save_info_fn):
    """pose_sweep.test (tools/final_common.py:107-174) with wide.sharded_shapley in place of the narrow call and no logits file."""
    folders = dict(selected_folders(args, get_folder_name_list(args)))
    model = load_model(args)
    write = iqdist.rank() == 0
    for pc_index, (data, lbl) in enumerate(stage1.data_loader(args)):
        if pc_index not in folders:
            continue
        data, lbl = data.to(args.device), lbl.to(args.device)
        base_folder = folders[pc_index]
        mode_folder = base_folder + "%s_all/" % args.mode
        region_id = np.load(base_folder + "region_id.npy")
        orders = load_orders(base_folder, args)
        io = None
        if write:
            mkdir(mode_folder)
            io = IOStream(mode_folder + "log.txt")
            io.cprint(str(args))
            io.cprint("norm factor: %f" % np.load(base_folder + "norm_factor.npy"))

        t_start = time.time()
        with torch.no_grad():
            all_params = get_transform_params_fn(args, data.device)
            n_pose = all_params.size()[0]
            poses = torch.cat([disturb_fn(data, all_params[i]) for i in range(n_pose)], dim=0)
            orig, phi = wide.sharded_shapley(model, data, poses, lbl, region_id, orders, args, route=args.route,
                                             coalitions=args.coalitions)
        if write:
            io.cprint("origin region shapley: %s" % str(orig))
            np.save(mode_folder + "orig_shapley_value.npy", orig)
            phi_np = phi.cpu().numpy()
            for i in range(n_pose):
                print_info_fn(io, all_params[i], phi_np[i], i)
            np.save(mode_folder + "region_shapley_value.npy", phi_np)
            save_info_fn(all_params, mode_folder)
            io.cprint("time: %f" % (time.time() - t_start))
            io.close()


def make_args(argv=None):
    parser = stage1.build_parser()
    parser.add_argument("--mode", choices=sorted(MODES), required=True)
    add_wide_flags(parser)
    args = stage1.parse_game_args(parser, argv, DEFAULT_REGIONS, MIN_REGIONS, wide.MAX_REGIONS,
                                  "the wide stage takes %d .. %d regions (final_{trans,rotate,scale}_center_enum_all.py: up to 64)"
                                  % (MIN_REGIONS, wide.MAX_REGIONS))
    args.angle_threshold, args.num_grid_enum_rotate = pose_sweep.ANGLE_THRESHOLD, pose_sweep.NUM_GRID_ENUM_ROTATE
    args.trans_dist_threshold, args.num_grid_enum_trans = pose_sweep.TRANS_DIST_THRESHOLD, pose_sweep.NUM_GRID_ENUM_TRANS
    args.scale_upper, args.scale_lower, args.num_grid_enum_scale = pose_sweep.SCALE_UPPER, pose_sweep.SCALE_LOWER, pose_sweep.NUM_GRID_ENUM_SCALE
    return args


def run(args):
    test(args, *MODES[args.mode])


@iqdist.record
def main(argv=None):
    args = make_args(argv)
    stage1.finish_args(args)
    check_wide_args(args)
    run(args)


if __name__ == "__main__":
    main()
