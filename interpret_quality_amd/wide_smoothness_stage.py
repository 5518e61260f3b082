"""final_wide_smoothness.py - stage 5 (smoothness.py, the mirror of final_smoothness_center_enum_all.py) for more than 64 regions, up
to one region per point: region Shapley values while the linearity / planarity / scattering of every region is pushed up ("inc")
or down ("dec"), on the region ids and the first ``--num_samples`` permutations that final_wide_shapley.py wrote for the same
``--num_regions``.

The three modes and both objectives run as smoothness.run / test_all_region run them, with the wide enumerator
(smoothness.enumerate_smoothness(wide=True): iq_smoothness_enum_wide, the narrow stage's kernel, one wave per region) and
``wide.sharded_shapley`` (the epochs' clouds sharded over the ranks, one gather, rank 0 writes).  Artefacts under
``<cloud>/<mode>_all/allregion_<inc|dec>/``:

    orig_shapley_value.npy (R,)   region_shapley_value.npy (P,R)   <mode>.npy (P,R) float64   data_smoothness.npy (P,1,N,3) float32
    log.txt (smoothness._log_enumeration)

No ``all_logits.pt`` (wide_pose_stage.py: the one deviation, for size).  A region of fewer than two points is left untouched,
smoothness NaN, stop_epoch -1, as in the narrow stage - above a few hundred regions that is common, and with one region per point no
region can move: the enumeration then yields one pose, the original cloud.  Clouds of at most 1024 points (a region's points live
in the kernel's LDS arrays); more is an IqError.
"""
import time

import numpy as np
import torch

from . import dist as iqdist
from . import hip_ops, smoothness, wide
from . import shapley_stage as stage1
from ._lib import IqError
from .final_util import IOStream, get_folder_name_list, load_model, mkdir
from .wide_pose_stage import add_wide_flags, check_wide_args, load_orders, selected_folders
from .wide_stage import DEFAULT_REGIONS, MIN_REGIONS


def test_all_region(model, data, lbl, orders, region_id, mode_folder, args, objective):
    """smoothness.test_all_region (final_smoothness_center_enum_all.py:280-356) for a wide game."""
    assert objective in ["inc", "dec"]
    if data.shape[1] > hip_ops.MAX_SMOOTHNESS_POINTS:
        raise IqError("the wide smoothness stage takes clouds of at most %d points, got N=%d" % (hip_ops.MAX_SMOOTHNESS_POINTS, data.shape[1]))
    t_start = time.time()
    write = iqdist.rank() == 0
    result_path = mode_folder + "allregion_%s/" % objective
    io = None
    if write:
        mkdir(result_path)
        io = IOStream(result_path + "log.txt")
        io.cprint(str(args))
    with torch.no_grad():
        poses, smoothness_list, res = smoothness.enumerate_smoothness(data, region_id, args, objective, wide=True)
        n_pose = poses.shape[0]
        orig_shap_value, phi = wide.sharded_shapley(model, data, poses, lbl, region_id, orders, args, route=args.route,
                                                    coalitions=args.coalitions)
    if write:
        io.cprint("origin shapley of this region: %s" % str(orig_shap_value))
        np.save(result_path + "orig_shapley_value.npy", orig_shap_value)
        smoothness._log_enumeration(io, res, n_pose, args, objective)
        phi_np = phi.cpu().numpy()
        for e in range(n_pose):
            io.cprint("epoch %d region shapley value: %s" % (e, str(phi_np[e])))
        np.save(result_path + "region_shapley_value.npy", phi_np)             # (num_poses, num_regions)
        np.save(result_path + "%s.npy" % args.mode, smoothness_list)           # (num_poses, num_regions)
        np.save(result_path + "data_smoothness.npy", poses.unsqueeze(1).cpu().numpy())  # (num_poses,1,N,3)
        io.cprint("time: %f" % (time.time() - t_start))
        io.close()


def test_smoothness(args, model):
    """smoothness.test_smoothness (:360-390) on the artefacts of the wide stage 1."""
    folders = dict(selected_folders(args, get_folder_name_list(args)))
    for pc_index, (data, lbl) in enumerate(stage1.data_loader(args)):
        if pc_index not in folders:
            continue
        data, lbl = data.to(args.device), lbl.to(args.device)
        base_folder = folders[pc_index]
        mode_folder = base_folder + "%s_all/" % args.mode
        region_id = np.load(base_folder + "region_id.npy")
        orders = load_orders(base_folder, args)
        test_all_region(model, data, lbl, orders, region_id, mode_folder, args, objective="inc")
        test_all_region(model, data, lbl, orders, region_id, mode_folder, args, objective="dec")


def make_args(argv=None):
    parser = stage1.build_parser("pointnet")
    add_wide_flags(parser)
    args = stage1.parse_game_args(parser, argv, DEFAULT_REGIONS, MIN_REGIONS, wide.MAX_REGIONS,
                                  "the wide stage takes %d .. %d regions (final_smoothness_center_enum_all.py: up to 64)"
                                  % (MIN_REGIONS, wide.MAX_REGIONS))
    args.step, args.enum_step, args.epoch = smoothness.STEP, smoothness.ENUM_STEP, smoothness.EPOCH
    args.var_threshold, args.dist_threshold = smoothness.VAR_THRESHOLD, smoothness.DIST_THRESHOLD
    args.stop_ratio, args.max_iteration = smoothness.STOP_RATIO, smoothness.MAX_ITERATION
    return args


def run(args):
    selected_folders(args, get_folder_name_list(args))      # fail before the model is built
    model = load_model(args)
    for mode in hip_ops.SMOOTHNESS_MODES:                    # final_smoothness_center_enum_all.py:413-418
        args.mode = mode
        test_smoothness(args, model)


@iqdist.record
def main(argv=None):
    args = make_args(argv)
    stage1.finish_args(args)
    check_wide_args(args)
    run(args)


if __name__ == "__main__":
    main()
