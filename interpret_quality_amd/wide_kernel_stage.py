"""final_wide_kernel_shapley.py - region Shapley values of a wide game (65 .. 1024 regions) by the regression (KernelSHAP) estimator
with the analytic Gram matrix (wide_kernelshap.py); kernel_stage.py is the stage for 2 .. 64 regions.

Per selected cloud, under the wide experiment folder of that region count (``exp_folder``; the folder final_wide_shapley.py uses):

    kernelshap/coalitions.npy                     (M, W) uint64  the sampled rows, bit (r & 63) of word (r >> 6) = region r kept
    kernelshap/rewards.npy                        (M,) float32   their rewards
    kernelshap/region_shapley_value.npy           (R,) float64   the estimate from all M rows
    kernelshap/running_counts.npy                 (k,) int64     row counts c (R + 1), c in stage 1's sample counts, <= M
    kernelshap/running_region_shapley_value.npy   (k, R) float64 the estimate from the first count rows
    kernelshap/draw.json                          {"draw", "seed", "stream"}: the contract that made the rows; with --pairs also
                                                  "pairs": true, with --se also "se": true
    kernelshap/region_interaction.npy             (R, R) float64 with --pairs: the SHAP-IQ estimate of the pairwise Shapley
                                                  interaction index of every pair of regions from the same M rows
                                                  (wide_kernelshap.pairs; symmetric, zero diagonal), no further model evaluation
    kernelshap/region_shapley_se.npy              (R,) float64   with --se: the standard error of region_shapley_value.npy
    kernelshap/region_interaction_se.npy          (R, R) float64 with --se and --pairs: the standard error of every entry of
                                                  region_interaction.npy (symmetric, zero diagonal)
    kernelshap/region_interaction_cv.npy          (R, R) float64 with --pairs and --control shift: SHAP-IQ on the rewards less the
                                                  additive game that spreads v_full - v_empty evenly (wide_kernelshap.pairs_cv;
                                                  DESIGN.md 5j), beside region_interaction.npy, which is still written
    kernelshap/region_interaction_cv_se.npy       (R, R) float64 its standard error
    kernelshap/control.json                       {"control", "ridge", "fold_rows", "paired"} of that estimate
    kernelshap/control_pairs.npy                  (K, 2) int32   with --control sparse: region_interaction_cv.npy is
                                                  then the cross-fitted surrogate of all R singles and these pairs, the
                                                  --control_pairs K (default min(3 R, 2080 - R)) nearest pairs of FPS centres, and
                                                  control.json {"control", "select", "pairs", "features", "fold_rows", "ridge", "status"}

``--samples`` is the number of rows M (model evaluations; default 1000 (R + 1), stage 1's budget).  The clouds, the FPS centres and
the region ids are final_wide_shapley.py's (wide_stage.cal_region_id).  The draws after the sizes come from the device sampler
whatever ``--sampler`` says (the contract of DESIGN.md 5f; the flag is taken because the wide stages share one set of flags), and
a cloud that is not selected performs the same draws, so what a cloud gets does not depend on which others are selected.  There is no exact
value at these region counts: where stage 1 has written the cloud's permutation estimate (region_shapley/<i>_<count>.npy), the
cloud's line gives the max and RMS difference to the one of the most permutations - a cross-check, not an error.  Single process:
under several ranks rank 0 does the work and the others wait at the end.

``--draw counter`` (default ``stream``, all of the above) draws the rows by the counter-based contract instead: row
m of cloud i is a function of (--seed, i, m, R) alone, so a cloud that is not selected draws nothing and NumPy's generator is not
touched.  draw.json's "stream" is the cloud's index under ``counter`` and null under ``stream``.
"""
import glob
import json
import os

import numpy as np
import torch

from . import dist as iqdist
from . import shapley_stage as stage1
from . import kernel_stage, wide_kernelshap, wide_stage
from .final_util import get_folder_name_list, load_model, mkdir

FILES = kernel_stage.FILES


def kernel_one_cloud(model, data, lbl, region_id, args, cloud=0, fps_index=None):
    """-> dict of one cloud's artefacts (kernel_stage.artefacts).  ``cloud``: its index, the key's second word under
    ``--draw counter``; ``fps_index``: its FPS centres, read by --control sparse alone."""
    return kernel_stage.artefacts(wide_kernelshap.game(model, data, lbl, region_id, args, args.samples, not args.unpaired,
                                                       coalitions=args.coalitions, draw=args.draw, seed=args.seed, stream=cloud,
                                                       pairs=kernel_stage.wants_pairs(args),
                                                       **({"se": True} if kernel_stage.wants_se(args) else {}),
                                                       **kernel_stage.control_arguments(args, data, fps_index)))


def stage1_estimate(result_path, i):
    """Stage 1's region_shapley/<i>_<count>.npy of the largest count there is -> (count, (R,) array), or None."""
    found = {}
    for path in glob.glob(result_path + "region_shapley/%d_*.npy" % i):
        count = os.path.basename(path)[:-4].split("_")[-1]
        if count.isdigit():
            found[int(count)] = path
    if not found:
        return None
    return max(found), np.load(found[max(found)])


def _skip_draw(result_path, args, save=False):
    """What a cloud that is not selected draws: the same sizes and permutations, nothing written; under ``--draw counter``
    nothing at all."""
    if args.draw == "counter":
        return
    samples = args.samples or wide_kernelshap.default_samples(args.num_regions)
    wide_kernelshap.draw(args.num_regions, samples, not args.unpaired, args.device, skip=True)


def run(args):
    model = load_model(args)
    with torch.no_grad():
        for i, name, result_path, data, lbl, fps_index in stage1.selected_clouds(args, get_folder_name_list(args), _skip_draw):
            mkdir(result_path + "kernelshap/")
            region_id = wide_stage.cal_region_id(data, fps_index, result_path, save=False)
            out = kernel_one_cloud(model, data, lbl, region_id, args, i, fps_index)
            kernel_stage.save(result_path + "kernelshap/", out)
            with open(result_path + "kernelshap/draw.json", "w") as f:
                json.dump({"draw": args.draw, "seed": int(args.seed), "stream": i if args.draw == "counter" else None,
                           **({"pairs": True} if kernel_stage.wants_pairs(args) else {}),
                           **({"se": True} if kernel_stage.wants_se(args) else {})}, f)
            phi = out["region_shapley_value"]
            line = "pointcloud:%s, index:%d, regions:%d, rows:%d, sum(phi)=%.6f, v_full - v_empty=%.6f" % (
                name, i, args.num_regions, out["coalitions"].shape[0], phi.sum(), out["v_full"] - out["v_empty"])
            other = stage1_estimate(result_path, i)
            if other is not None and other[1].shape == phi.shape:
                diff = phi - other[1]
                line += ", against %d permutations: max difference %.4g, rms %.4g" % (
                    other[0], np.abs(diff).max(), np.sqrt((diff ** 2).mean()))
            print(line)


def make_args(argv=None):
    parser = stage1.build_parser()
    wide_stage.add_wide_flags(parser, route=False)
    kernel_stage.add_sample_flags(parser)
    parser.add_argument("--draw", choices=wide_kernelshap.DRAWS, default="stream",
                        help="how the rows are drawn: from NumPy's MT19937 stream (default), or counter-based (Philox keyed by "
                             "--seed and the cloud's index): any cloud alone, no skip draws")
    kernel_stage.add_pairs_flag(parser)
    kernel_stage.add_se_flag(parser)
    kernel_stage.add_control_flag(parser, wide_kernelshap.CONTROLS)
    args = wide_stage.parse_wide_args(parser, argv, "final_kernel_shapley.py", samples=False)
    kernel_stage.check_samples(parser, args)
    kernel_stage.check_se(parser, args, "analytic")
    kernel_stage.check_control(parser, args)
    return args


@iqdist.record
def main(argv=None):
    args = make_args(argv)
    stage1.finish_args(args)
    wide_stage.check_points(args)
    stage1.rank0_only(run, args, "wide kernelshap")


if __name__ == "__main__":
    main()
