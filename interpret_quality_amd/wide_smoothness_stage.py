"""final_wide_smoothness.py - stage 5 (smoothness.py, the mirror of final_smoothness_center_enum_all.py) for more than 64 regions, up
to one region per point: region Shapley values while the linearity / planarity / scattering of every region is pushed up ("inc")
or down ("dec"), on the region ids and the first ``--num_samples`` permutations that final_wide_shapley.py wrote for the same
``--num_regions``.

The three modes and both objectives run through smoothness.run_modes / test_all_region, the narrow stage's own loops: this file is
the parser, and ``run`` hands them the wide game (wide_stage.GAME: stage 1's files checked, the first ``--num_samples``
permutations, ``wide.sharded_shapley`` - the epochs' clouds sharded over the ranks, one gather, rank 0 writes) and the wide
enumerator (smoothness.enumerate_smoothness(wide=True): iq_smoothness_enum_wide, the narrow stage's kernel, one wave per region).
Artefacts under
``<cloud>/<mode>_all/allregion_<inc|dec>/``:

    orig_shapley_value.npy (R,)   region_shapley_value.npy (P,R)   <mode>.npy (P,R) float64   data_smoothness.npy (P,1,N,3) float32
    log.txt (smoothness._log_enumeration)

No ``all_logits.pt`` (wide_pose_stage.py: the one deviation, for size).  A region of fewer than two points is left untouched,
smoothness NaN, stop_epoch -1, as in the narrow stage - above a few hundred regions that is common, and with one region per point no
region can move: the enumeration then yields one pose, the original cloud.  Clouds of at most 1024 points (a region's points live
in the kernel's LDS arrays); more is an IqError of hip_ops.smoothness_enum_wide that names the point count.
"""
import functools

from . import dist as iqdist
from . import shapley_stage as stage1
from . import smoothness, wide_stage
from .final_util import get_folder_name_list


def make_args(argv=None):
    parser = stage1.build_parser("pointnet")
    wide_stage.add_wide_flags(parser, num_samples=True)
    return smoothness.set_enum_args(wide_stage.parse_wide_args(parser, argv, "final_smoothness_center_enum_all.py"))


def run(args):
    wide_stage.selected_folders(args, get_folder_name_list(args))      # fail before the model is built
    smoothness.run_modes(args, wide_stage.GAME, functools.partial(smoothness.enumerate_smoothness, wide=True))


@iqdist.record
def main(argv=None):
    args = make_args(argv)
    stage1.finish_args(args)
    wide_stage.check_wide_args(args)
    run(args)


if __name__ == "__main__":
    main()
