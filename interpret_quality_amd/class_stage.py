"""final_class_shapley.py - region Shapley values for EVERY class (or the classes named) from one pass over a game's coalitions
(classwise.py; the reference scores the ground-truth label only).

The stage runs on the experiment folder stage 1 wrote for that region count - final_shapley_value.py up to 64 regions,
final_wide_shapley.py above - and reads each selected cloud's region_id.npy and, for the permutation estimator, the first
``--num_samples`` rows of its all_orders.npy.  Per cloud it writes into ``<cloud>/classwise/``:

    region_shapley_classes.npy   (G, R) float64   row g: the Shapley values of the game of label classes[g]
    efficiency.npy               (G,) float64     sum_r phi[g][r] - (v_full[g] - v_empty[g])
    region_shapley_classes_se.npy (G, R) float64  with --se: the standard error of every entry of region_shapley_classes.npy, from
                                 the second moment of the same coalitions' rewards; classes.json gains "se": true
    classes.json                 the labels, the ground-truth label, the argmax class of the full cloud, v_full and v_empty per
                                 class, the estimator and its parameters

``--estimator permutation`` (default) walks stage 1's permutations: the ground-truth row is stage 1's
region_shapley/<i>_<count>.npy at ``--num_samples`` = count, bit for bit, and nothing is drawn from NumPy's global generator.
``--estimator kernel`` is the regression estimator on ``--samples`` rows (``--draw stream``: NumPy's stream, which runs on from
one selected cloud to the next; above 64 regions also ``--draw counter``, keyed by --seed and the cloud's index).  Above 64
regions ``--route`` and ``--coalitions`` are wide.shapley's.  ``--se`` with the kernel estimator follows final_kernel_shapley.py's
rule: phi has a standard error under the analytic Gram matrix only, which this stage uses above 64 regions.  One rank: the stage is not sharded and refuses a larger world.
"""
import json

import numpy as np
import torch

from . import classwise, kernel_stage
from . import dist as iqdist
from . import shapley_stage as stage1
from . import wide, wide_kernelshap, wide_stage
from .final_util import NUM_REGIONS, NUM_SAMPLES, get_folder_name_list, load_model, mkdir

ESTIMATORS = ("permutation", "kernel")
MIN_REGIONS = 2
FOLDER = "classwise/"


def parse_classes(text):
    """``--classes``: "all" -> None, "0,3,7" -> [0, 3, 7]; ValueError otherwise."""
    if text == "all":
        return None
    labels = [int(t) for t in text.split(",")]       # int(): ValueError for an empty or non-numeric field
    if not 1 <= len(labels) <= classwise.MAX_CLASSES or min(labels) < 0:
        raise ValueError(text)
    return labels


def first_stage(args):
    """The script that writes the folder this stage reads."""
    return "final_shapley_value.py" if args.num_regions <= classwise.NARROW_REGIONS else "final_wide_shapley.py"


def cloud_files(base, args):
    """region_id.npy and, for the permutation estimator, the first --num_samples permutations of one cloud's folder ``base``;
    SystemExit naming the stage to run first when a file is missing."""
    needed = ("region_id.npy",) + (("all_orders.npy",) if args.estimator == "permutation" else ())
    for f in needed:
        wide_stage.require(base + f, args, first_stage(args))
    region_id = np.load(base + "region_id.npy")
    orders = wide_stage.load_orders(base, args) if args.estimator == "permutation" else None
    return region_id, orders


def class_one_cloud(model, data, region_id, orders, args, cloud=0):
    """-> (phi (G,R) float64, v_full (G,), v_empty (G,), the full cloud's logits (C,)) of one cloud; with --se a fifth value,
    the (G,R) standard error of phi."""
    wide_game = args.num_regions > classwise.NARROW_REGIONS
    route, coalitions = (args.route, args.coalitions) if wide_game else (None, None)
    se = {"se": True} if kernel_stage.wants_se(args) else {}
    if args.estimator == "permutation":
        _, total, *bars = classwise.shapley(model, data, region_id, orders, args, args.class_list, route=route, coalitions=coalitions, **se)
        phi = total / orders.shape[0]
    else:
        phi, _, _, *bars = classwise.kernel_shapley(model, data, region_id, args, args.class_list, args.samples,
                                                    draw=args.draw if wide_game else "stream", seed=args.seed, stream=cloud,
                                                    coalitions=coalitions, **se)
    v_full, v_empty, logits = classwise.ends(model, data, region_id, args, args.class_list, coalitions)
    return (phi, v_full, v_empty, logits) + tuple(bars)


def run(args):
    model = load_model(args)
    names = get_folder_name_list(args)
    with torch.no_grad():
        for i, (data, lbl) in enumerate(stage1.data_loader(args)):
            if not iqdist.cloud_selected(args, i):
                continue
            base = args.exp_folder + "%s/" % names[i]
            region_id, orders = cloud_files(base, args)
            phi, v_full, v_empty, logits, *bars = class_one_cloud(model, data.to(args.device), region_id, orders, args, i)
            labels = list(range(logits.shape[0])) if args.class_list is None else args.class_list
            eff = phi.sum(axis=1) - (v_full - v_empty)
            mkdir(base + FOLDER)
            np.save(base + FOLDER + "region_shapley_classes.npy", phi)
            np.save(base + FOLDER + "efficiency.npy", eff)
            if bars:
                np.save(base + FOLDER + "region_shapley_classes_se.npy", bars[0])
            params = {"num_regions": int(args.num_regions), "softmax_type": args.softmax_type}
            if args.estimator == "permutation":
                params.update(num_samples=int(orders.shape[0]), route=args.route, coalitions=args.coalitions)
            else:
                params.update(samples=args.samples, draw=args.draw, seed=int(args.seed), coalitions=args.coalitions)
            with open(base + FOLDER + "classes.json", "w") as f:
                json.dump({"classes": [int(c) for c in labels], "label": int(lbl.reshape(-1)[0]), "predicted": int(np.argmax(logits)),
                           "v_full": [float(x) for x in v_full], "v_empty": [float(x) for x in v_empty],
                           "estimator": args.estimator, "parameters": params, **({"se": True} if bars else {})}, f)
            print("pointcloud:%s, index:%d, regions:%d, classes:%d, label:%d, predicted:%d, max |efficiency gap| %.3g"
                  % (names[i], i, args.num_regions, phi.shape[0], int(lbl.reshape(-1)[0]), int(np.argmax(logits)), np.abs(eff).max()))


def build_parser():
    parser = stage1.build_parser()
    parser.add_argument("--estimator", choices=ESTIMATORS, default="permutation")
    parser.add_argument("--classes", type=str, default="all", help="all, or labels separated by commas: 0,3,7 (any order, repeats allowed)")
    parser.add_argument("--num_samples", type=int, default=NUM_SAMPLES,
                        help="permutation estimator: the first rows of the all_orders.npy that stage 1 wrote")
    parser.add_argument("--route", choices=wide.ROUTES, default=None, help="above 64 regions: wide.shapley's route")
    parser.add_argument("--coalitions", choices=wide.COALITIONS, default=None, help="above 64 regions: how a family other than PointNet "
                        "evaluates the coalitions")
    parser.add_argument("--samples", type=int, default=None, help="kernel estimator: coalition rows per cloud; default 1000 (num_regions + 1)")
    parser.add_argument("--draw", choices=wide_kernelshap.DRAWS, default="stream", help="kernel estimator above 64 regions: how the rows are drawn")
    kernel_stage.add_se_flag(parser)
    return parser


def make_args(argv=None):
    parser = build_parser()
    args = stage1.parse_game_args(parser, argv, NUM_REGIONS, MIN_REGIONS, wide.MAX_REGIONS,
                                  "the class-wise stage takes %d .. %d regions" % (MIN_REGIONS, wide.MAX_REGIONS), samples=False)
    try:
        args.class_list = parse_classes(args.classes)
    except ValueError:
        parser.error("--classes %r: all, or at most %d labels >= 0 separated by commas" % (args.classes, classwise.MAX_CLASSES))
    narrow = args.num_regions <= classwise.NARROW_REGIONS
    if narrow and (args.route is not None or args.coalitions is not None or args.draw != "stream"):
        parser.error("--route, --coalitions and --draw belong to games of more than %d regions" % classwise.NARROW_REGIONS)
    if args.num_samples < 1:
        parser.error("--num_samples %d: at least one permutation" % args.num_samples)
    kernel_stage.check_samples(parser, args)
    if kernel_stage.wants_se(args):
        if args.estimator == "permutation" and args.num_samples < 2:
            parser.error("--se with --num_samples %d: a standard error needs at least 2 permutations" % args.num_samples)
        if args.estimator == "kernel" and narrow:
            parser.error("--se with --estimator kernel at %d regions: this stage solves with the sampled Gram matrix up to %d "
                         "regions, and phi has a standard error under the analytic one only (final_kernel_shapley.py --gram "
                         "analytic --se)" % (args.num_regions, classwise.NARROW_REGIONS))
    return args


@iqdist.record
def main(argv=None):
    args = make_args(argv)
    stage1.finish_args(args)
    if iqdist.world() > 1:
        raise SystemExit("final_class_shapley.py runs on one rank (it is not sharded): got a world of %d" % iqdist.world())
    wide_stage.check_points(args)
    run(args)


if __name__ == "__main__":
    main()
