"""final_wide_interaction.py - the multi-order interactions (scripts/exp_interaction.sh: final_gen_pair.py,
final_point_binary_interaction_logits.py, final_cal_interactions.py) for more than 64 regions, up to one region per point.

For every cloud in the interaction selection of the dataset it reads ``region_id.npy`` from the experiment folder that
final_wide_shapley.py wrote for ``--num_regions`` and writes, under the reference's names and layout:

    interaction_seed<k>/region_pair_list.npy                        (num_pairs_random, 2) int64
    interaction_seed<k>/ratio<r>_context_list.npy                   (P, C, m) int16, m = int((R-2) * ratio)
    interaction_seed<k>/normal/ratio<r>_all_logits.pt               (P, 4C, K) float32
    interaction_seed<k>/normal/ratio<r>_<output_type>_interaction.npy   (P, C) float64

and, with ``--transform_params FILE.npy`` (the angle tuple or translation vector of ``--mode``), the same pairs and contexts on the
perturbed cloud into ``interaction_seed<k>/<mode>_adv/`` (with transform_params.npy and pred_labels.npy, as final_gen_pair.py
leaves them there).  ``--adv_pose sweep`` finds that pose itself: for each selected cloud it reads the parameter file that
final_wide_pose.py --mode <mode> wrote (``<mode>_all/trans_vector.npy`` | ``angle_tuple.npy``), picks the pose with the lowest reward
on the true class by one dense forward over all poses (gen_pair.lowest_reward_pose: check_adv_success's rule and code), writes
``pose_idx.npy`` and ``transform_params.npy`` into ``<mode>_adv/`` and evaluates that pose exactly as ``--transform_params`` with that
row would.  The two flags exclude each other.

Deviations from the reference, both for size: the context lists are saved in the narrowest integer type that holds R (int16; at
R = 1024 the reference's int64 would be 1.4 GB per cloud - nothing but this driver reads these files), and pairs and contexts are
saved for the selected clouds only.  The random stream is final_gen_pair.py's for ``--seed <k>``: NumPy's global generator, seeded
with ``--gen_pair_seed``, draws the pairs of ALL clouds first and then the contexts of all clouds, selected or not - on the host,
or with ``--sampler device`` the pairs on the host and the contexts on the GPU (wide.iter_contexts with a device: the same stream,
the same files byte for byte; the contexts of a cloud that is not selected are passed over without being written).  Not here
(DESIGN.md 5e): the single-region folders of final_gen_pair.py (at R = 128 there are 128 of them, each with its own contexts) and
sharding over ranks - under several ranks rank 0 does the work and the others wait.
"""
import numpy as np
import torch

from . import dist as iqdist
from . import gen_pair, interaction, wide
from .final_util import get_folder_name_list, load_model, mkdir, set_random
from .pose_sweep import rotate_xyz, translate_pc
from .shapley_stage import finish_args, rank0_only
from .wide_stage import add_wide_flags, check_points, parse_wide_args, require

CONTEXT_DTYPE = np.int16      # holds every region id of a wide game (wide.MAX_REGIONS = 1024)


def _folder(args, name):
    return args.exp_folder + "%s/" % name + "interaction_seed%d/" % args.gen_pair_seed


def _wanted(args, names):
    """Indices of the clouds this call computes: the interaction selection, within ``args.cloud_subset`` and the loader."""
    return [i for i in interaction._selected(args) if i < len(names) and iqdist.cloud_selected(args, i)]


def draw(args, names, wanted):
    """The pairs of all clouds, then the contexts of all clouds (gen_pair.run's order); saved for the clouds of ``wanted``."""
    pairs = [wide.gen_pair_random(args) for _ in names]
    last = max(wanted)           # nothing later in this call reads the stream: the contexts of the clouds after it are not drawn
    dev = args.device if getattr(args, "sampler", "host") == "device" else None     # --sampler device: the same stream on the GPU
    for i in range(last + 1):
        folder = _folder(args, names[i])
        if i in wanted:
            mkdir(folder + "normal/")
            np.save(folder + "region_pair_list.npy", pairs[i])
        elif dev is not None:    # passed over in the sampler's skip mode: nothing is written, nothing comes to the host
            wide.skip_contexts(len(pairs[i]), args.num_regions, args.ratio, args.num_save_context_max, dev)
            continue
        contexts = wide.iter_contexts(pairs[i], args.num_regions, args.ratio, args.num_save_context_max, dtype=CONTEXT_DTYPE,
                                      device=dev)
        for ratio, context_list in zip(args.ratio, contexts):      # one ratio resident at a time
            if i in wanted:
                np.save(folder + "ratio%d_context_list.npy" % int(ratio * 100), context_list)


def _sweep_params_path(args, base_folder):
    """The parameter file of the cloud's wide pose sweep of ``args.mode`` (wide_pose_stage.py)."""
    return base_folder + "%s_all/" % args.mode + ("trans_vector.npy" if args.mode == "trans" else "angle_tuple.npy")


def evaluate(model, data, lbl, region_id, folder, save_path, args):
    """save_logits_all_orders + cal_interaction_all_orders (final_point_binary_interaction_logits.py:73-80,
    final_cal_interactions.py:40-46) for one pose of one cloud."""
    mkdir(save_path)
    pairs = np.load(folder + "region_pair_list.npy")
    for ratio in args.ratio:
        tag = int(ratio * 100)
        context_list = np.load(folder + "ratio%d_context_list.npy" % tag)
        all_logits = wide.interaction_logits(model, data, region_id, pairs, context_list, args,
                                             coalitions=args.coalitions)
        torch.save(all_logits, save_path + "ratio%d_all_logits.pt" % tag)
        np.save(save_path + "ratio%d_%s_interaction.npy" % (tag, args.output_type), wide.interactions(all_logits, lbl, args))
        print("\tratio: %f, logits %s" % (ratio, tuple(all_logits.shape)))


def run(args):
    names = get_folder_name_list(args)
    wanted = _wanted(args, names)
    if not wanted:
        return
    for i in wanted:
        require(args.exp_folder + "%s/region_id.npy" % names[i], args)
        if args.adv_pose == "sweep":
            require(_sweep_params_path(args, args.exp_folder + "%s/" % names[i]), args, "final_wide_pose.py --mode %s" % args.mode)
    model = load_model(args)
    disturb_fn = translate_pc if args.mode == "trans" else rotate_xyz
    params = np.load(args.transform_params) if args.transform_params else None
    set_random(args.gen_pair_seed)        # final_gen_pair.py --seed <k> writes interaction_seed<k>/
    draw(args, names, wanted)
    with torch.no_grad():
        for _, _, data, lbl, base_folder, folder, _ in interaction.selected_clouds(args):
            region_id = np.load(base_folder + "region_id.npy")
            print("##### normal pose")
            evaluate(model, data, lbl, region_id, folder, folder + "normal/", args)
            adv = folder + "%s_adv/" % args.mode
            if args.adv_pose == "sweep":
                sweep = np.load(_sweep_params_path(args, base_folder))
                pose_idx = gen_pair.lowest_reward_pose(model, data, lbl, sweep, disturb_fn, args)
                print("Pose idx with max attacking utility: %d" % pose_idx)
                mkdir(adv)
                np.save(adv + "pose_idx.npy", pose_idx)
                params = sweep[pose_idx]
            if params is None:
                continue
            print("##### %s pose of %s" % (args.mode, "the sweep" if args.adv_pose else "--transform_params"))
            mkdir(adv)
            np.save(adv + "transform_params.npy", params)
            gen_pair.gen_pred_label(model, data, lbl, disturb_fn, adv, args)
            pred = torch.tensor([np.load(adv + "pred_labels.npy")[1]], dtype=torch.long, device=args.device)
            data_disturb = disturb_fn(data, torch.from_numpy(params.astype(np.float32)).to(args.device))
            evaluate(model, data_disturb, lbl if args.output_type == "gt" else pred, region_id, folder, adv, args)


def make_args(argv=None):
    parser = interaction.build_parser(with_cal_flags=True)
    parser.set_defaults(device_id=0)
    parser.add_argument("--transform_params", type=str, default=None, metavar="FILE.npy",
                        help="the --mode parameters of one pose: the same pairs and contexts are also evaluated there")
    parser.add_argument("--adv_pose", choices=("sweep",), default=None,
                        help="sweep: take the adversarial pose from the wide pose sweep of --mode (the pose with the lowest reward "
                             "on the true class) instead of --transform_params")
    add_wide_flags(parser, route=False)
    args = parse_wide_args(parser, argv, "final_gen_pair.py and final_point_binary_interaction_logits.py", samples=False)
    if args.adv_pose and args.transform_params:
        parser.error("--adv_pose sweep finds the pose itself: it cannot be combined with --transform_params")
    if args.mode not in ("rotate", "trans"):
        parser.error("--mode %s: rotate or trans" % args.mode)
    if args.num_save_context_max < 1 or args.num_pairs_random < 1:
        parser.error("--num_save_context_max and --num_pairs_random must be at least 1")
    return args


@iqdist.record
def main(argv=None):
    args = make_args(argv)
    finish_args(args)
    check_points(args)
    rank0_only(run, args, "wide")


if __name__ == "__main__":
    main()
