"""final_wide_pose.py --mode trans|rotate|scale - stages 2-4 (pose_sweep.py, the mirror of final_{trans,rotate,scale}_center_enum_all.py)
for more than 64 regions, up to one region per point: region Shapley values of every selected cloud under 216 translations / 216
rotations / 30 scales, on the region ids and the first ``--num_samples`` permutations that final_wide_shapley.py wrote for the same
``--num_regions``.

Grids, perturbations, the log / save helpers and the per-cloud loop are pose_sweep's own: this file is the parser, and ``run`` hands
pose_sweep.test the wide game (wide_stage.GAME: stage 1's files checked, the first ``--num_samples`` permutations,
``wide.sharded_shapley``) - the poses (and the original cloud as pose 0) sharded over the ranks, one gather per
cloud, rank 0 writes.  Every pose goes through the existing wide coalition entries (wide.py); there is no second evaluation path.
Artefacts per selected cloud under ``<exp_folder of R>/<cloud>/<mode>_all/``:

    orig_shapley_value.npy (R,)   region_shapley_value.npy (P,R) float64   trans_vector.npy + trans_distance.npy | angle_tuple.npy |
    scale.npy   log.txt

The one deviation from the narrow stage: no ``all_logits.pt``.  It is (P, S(R+1), C) - 0.45 GB per sweep at R = 128 and 3.5 GB at
R = 1024 with 100 permutations - and nothing downstream reads it (final_gen_pair.py and final_result.py read
region_shapley_value.npy and the parameter files only).
"""
from . import dist as iqdist
from . import pose_sweep
from . import shapley_stage as stage1
from . import wide_stage
from .final_util import get_folder_name_list
from .wide_stage import load_orders, selected_folders  # noqa: F401  (their home is wide_stage.py; the old names still import)

MODES = pose_sweep.MODES


def make_args(argv=None):
    parser = stage1.build_parser()
    parser.add_argument("--mode", choices=sorted(MODES), required=True)
    wide_stage.add_wide_flags(parser, num_samples=True)
    return pose_sweep.set_grid_args(wide_stage.parse_wide_args(parser, argv, "final_{trans,rotate,scale}_center_enum_all.py"))


def run(args):
    wide_stage.selected_folders(args, get_folder_name_list(args))      # fail before the model is built
    pose_sweep.test(args, *MODES[args.mode], game=wide_stage.GAME)


@iqdist.record
def main(argv=None):
    args = make_args(argv)
    stage1.finish_args(args)
    wide_stage.check_wide_args(args)
    run(args)


if __name__ == "__main__":
    main()
