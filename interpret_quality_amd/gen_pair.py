"""Stage 1 of scripts/exp_interaction.sh - host-side mirror of final_gen_pair.py: which region pairs
and which contexts the interaction stages evaluate, and which pose is "adversarial".

Everything random here is HOST NumPy on the global RNG, called in the reference's order, so for the
same seed the artefacts (region_pair_list.npy, ratio*_context_list.npy) are the reference's.  The
only device work is two dense forwards: all poses of a cloud in one batch (check_adv_success,
final_gen_pair.py:221-286) and the prediction at a chosen pose (gen_pred_label, :74-88).
"""
import argparse
import itertools

import numpy as np
import torch
from scipy.special import comb

from . import final_common, work
from .final_util import (BALL_QUERY_COEF, ball_query, cal_rank, get_folder_name_list, load_model, mkdir,
                         square_distance_np)  # noqa: F401
from .interaction import DEFAULT_RATIOS, _region_folders
from .pose_sweep import rotate_xyz, translate_pc
from . import dist as iqdist
from .shapley_stage import data_loader, finish_args, rank0_only


def gen_context(region_pair_list, save_path, args):
    """final_gen_pair.py:18-43.  For every ratio: m = int((R-2)*ratio) context regions per sample; at
    most num_save_context_max sampled contexts per pair, all C(R-2, m) of them when there are fewer.

    The reference draws every sampled context with np.random.choice(rest, m, replace=False) - the first m entries of a fresh
    np.random.permutation(R - 2) - on the global generator: 330 000 draws of 29 numbers for 300 pairs, 2.5 s of host time per
    cloud.  With ``args.device`` set the SAME stream is continued on the device (iq_sample_permutations, bit-identical, one
    launch per ratio) and handed back to NumPy; without it (host-only callers) the reference's loop runs on the host
    (``iter_contexts``)."""
    dev = getattr(args, "device", None)
    if dev is not None and getattr(dev, "type", None) == "cuda" and len(region_pair_list) > 0:
        return _gen_context_device(np.asarray(region_pair_list).reshape(-1, 2), save_path, args, dev)
    for ratio, context_list in zip(args.ratio, iter_contexts(region_pair_list, args.num_regions, args.ratio, args.num_save_context_max)):
        if len(region_pair_list) == 0:
            context_list = np.array([])     # what the reference's np.array(per_pair) makes of no pairs: (0,) float64
        print(context_list.shape)
        np.save(save_path + "ratio%d_context_list.npy" % int(ratio * 100), context_list)


def _rest(pairs, num_regions):
    """(P, R-2): per pair the regions outside it, ascending, as the reference's all_S."""
    regions = np.arange(int(num_regions))
    return [regions[(regions != i) & (regions != j)] for i, j in pairs]


def _enumerated(rest, m, dtype):
    """All C(R-2, m) contexts of one pair, in itertools' order."""
    listed = list(itertools.combinations(rest.tolist(), m))
    return np.array(listed, dtype=dtype).reshape(len(listed), m)


def iter_contexts(pairs, num_regions, ratios, num_save_context_max, dtype=None):
    """The reference's host loop (final_gen_pair.py:18-43), one ratio at a time: a generator of (P, C, m) arrays, drawn from
    NumPy's GLOBAL generator in the reference's order (ratio, pair, context).  ``dtype`` None: what the reference's
    np.array(per_pair) gives - int64, and float64 for the one empty context of m = 0.  wide.iter_contexts is this loop for up to
    wide.MAX_REGIONS regions."""
    r, cmax = int(num_regions), int(num_save_context_max)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    for ratio in ratios:
        m = int((r - 2) * ratio)
        sampled = comb(r - 2, m) > cmax
        per_pair = []
        for rest in _rest(pairs, r):
            if sampled:
                # np.random.choice(rest, m, replace=False) on the legacy generator: the head of a fresh permutation
                per_pair.append(np.array([rest[np.random.permutation(rest.size)[:m]] for _ in range(cmax)], dtype=dtype).reshape(cmax, m))
            else:
                per_pair.append(_enumerated(rest, m, dtype))
        yield np.stack(per_pair) if per_pair else np.zeros((0, 0, m), dtype=dtype)


def iter_contexts_device(pairs, num_regions, ratios, num_save_context_max, dev, draw, dtype=None, skip=False):
    """``iter_contexts`` with the sampled ratios drawn on the device, the one loop of the narrow and the wide stage: NumPy's global
    generator goes to the device once before the ratios, runs through the sampled ones in the reference's order and comes back
    once after the last of them (one sync), so that whatever the host draws next continues the reference's stream.
    ``draw(state, pairs, m)`` -> the (P, C, m) host array of one sampled ratio's contexts (the sampler call and the ``rest``
    mapping: what differs between narrow and wide).  The enumerated ratios come from itertools.combinations as on the host.
    ``skip``: the caller only passes the stream over - ``draw`` returns None, and nothing is enumerated either."""
    from . import hip_ops
    r, cmax = int(num_regions), int(num_save_context_max)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    ms = [int((r - 2) * ratio) for ratio in ratios]
    sampled = [comb(r - 2, m) > cmax for m in ms]
    left = sum(sampled)
    state = hip_ops.mt_state_to_device(dev) if left else None
    rest = None
    for m, is_sampled in zip(ms, sampled):
        if is_sampled:
            out = draw(state, pairs, m)
            left -= 1
            if left == 0:
                hip_ops.mt_state_to_host(state, set_global=True)
        elif skip:
            out = None
        else:
            rest = _rest(pairs, r) if rest is None else rest
            out = np.stack([_enumerated(row, m, dtype) for row in rest])
        yield out


def _gen_context_device(pairs, save_path, args, dev):
    from . import hip_ops
    n_rest, cmax, p = args.num_regions - 2, args.num_save_context_max, pairs.shape[0]
    rest = np.stack(_rest(pairs, args.num_regions))                                         # (P, R-2)

    def draw(state, pairs, m):
        first = hip_ops.sample_permutations(state, p * cmax, n_rest).cpu().numpy().astype(np.int64).reshape(p, cmax, n_rest)[:, :, :m]
        return np.take_along_axis(rest[:, None, :], first, axis=2)                          # rest[perm[:m]]

    contexts = iter_contexts_device(pairs, args.num_regions, args.ratio, cmax, dev, draw)
    for ratio, context_list in zip(args.ratio, contexts):
        print(context_list.shape)
        np.save(save_path + "ratio%d_context_list.npy" % int(ratio * 100), context_list)


def gen_pair_random(args):
    """final_gen_pair.py:288-300: num_pairs_random distinct unordered pairs (i < j)."""
    all_pairs = np.array([[i, j] for i in range(args.num_regions) for j in range(args.num_regions) if j > i])
    return all_pairs[np.random.choice(all_pairs.shape[0], size=args.num_pairs_random, replace=False)]


def gen_pair_single_region(region, neighbor_idx, args):
    """final_gen_pair.py:127-142: (region, neighbour) for every ball-query neighbour except itself."""
    neighbors = np.arange(args.num_regions)[neighbor_idx[region]]
    return np.array([[region, n] for n in neighbors if n != region])


def _interaction_folder(args, name):
    return args.exp_folder + "%s/" % name + "interaction_seed%d/" % args.seed


def save_pair_random(args, folder_name_list):
    """final_gen_pair.py:302-320."""
    print("gen pair random...")
    for name in folder_name_list:
        folder = _interaction_folder(args, name)
        mkdir(folder + "normal/")
        mkdir(folder + "%s_adv/" % args.mode)
        np.save(folder + "region_pair_list.npy", gen_pair_random(args))


def _dense_logits(model, clouds_cf, args):
    work.add(clouds_cf.shape[0])
    out = model(clouds_cf)
    return out[0] if args.model == "pointnet" else out


def lowest_reward_pose(model, data, lbl, params, disturb_fn, args):
    """The rule of check_adv_success (final_gen_pair.py:245-276) for one cloud: one dense forward over the poses ``params`` (P,3) of
    ``data`` (1,N,3); -> the index of the pose with the lowest reward on the true class.  Shared with the wide interaction stage."""
    poses = torch.cat([disturb_fn(data, torch.from_numpy(params[i]).to(args.device)) for i in range(params.shape[0])], dim=0)
    logits = _dense_logits(model, poses.permute(0, 2, 1).contiguous(), args)
    pred = torch.argmax(logits, dim=1)
    print("%d poses are misclassified" % int((pred != lbl[0].item()).sum()))
    v = final_common.get_reward(logits, lbl, args)
    return torch.argmin(v).item()


def check_adv_success(args, disturb_fn, folder_name_list):
    """final_gen_pair.py:221-286: one dense forward over all poses of each cloud; saves the pose with the
    lowest reward on the true class (max attacking utility)."""
    model = load_model(args)
    with torch.no_grad():
        for pc_idx, (data, lbl) in enumerate(data_loader(args)):
            name = folder_name_list[pc_idx]
            data, lbl = data.to(args.device), lbl.to(args.device)
            base_folder = args.exp_folder + "%s/" % name
            mode_folder = base_folder + "%s_all/" % args.mode
            params = np.load(mode_folder + ("trans_vector.npy" if args.mode == "trans" else "angle_tuple.npy"))
            pose_idx = lowest_reward_pose(model, data, lbl, params, disturb_fn, args)
            folder = _interaction_folder(args, name) + "%s_adv/" % args.mode
            np.save(folder + "pose_idx.npy", pose_idx)
            np.save(folder + "transform_params.npy", params[pose_idx])
            print("Pose idx with max attacking utility: %d" % pose_idx)


def save_pair_single_region(args, folder_name_list):
    """final_gen_pair.py:145-218: per region, the poses of its largest / smallest Shapley value and the
    pairs (region, neighbour) inside a ball of BALL_QUERY_COEF x cloud diameter around the region centre."""
    print("gen pair single region...")
    assert args.mode == "trans" or args.mode == "rotate"
    for pc_idx, (data, _) in enumerate(data_loader(args)):
        name = folder_name_list[pc_idx]
        pts = data.cpu().numpy().squeeze()
        base_folder = args.exp_folder + "%s/" % name
        mode_folder = base_folder + "%s_all/" % args.mode
        single = _interaction_folder(args, name) + "%s_adv_single_region/" % args.mode
        mkdir(single)
        region_id = np.load(base_folder + "region_id.npy")
        phi = np.load(mode_folder + "region_shapley_value.npy")                 # (num_poses, R)
        params = np.load(mode_folder + ("trans_vector.npy" if args.mode == "trans" else "angle_tuple.npy"))
        max_pose, min_pose = np.argmax(phi, axis=0), np.argmin(phi, axis=0)
        range_rank = args.num_regions - cal_rank(np.max(phi, axis=0) - np.min(phi, axis=0))  # 1 = largest range
        diameter = np.sqrt(np.maximum(square_distance_np(pts), 0)).max()
        centers = np.stack([pts[region_id == r].mean(axis=0) for r in range(args.num_regions)])
        neighbor_idx = ball_query(centers, r=BALL_QUERY_COEF * diameter)
        for region in range(args.num_regions):
            folder = single + "range_rank%02d_region%02d/" % (range_rank[region], region)
            for sub in ("normal/", "max_pose/", "min_pose/"):
                mkdir(folder + sub)
            np.save(folder + "max_pose/transform_params.npy", params[max_pose[region]])
            np.save(folder + "max_pose/pose_idx.npy", max_pose[region])
            np.save(folder + "min_pose/transform_params.npy", params[min_pose[region]])
            np.save(folder + "min_pose/pose_idx.npy", min_pose[region])
            pairs = gen_pair_single_region(region, neighbor_idx, args)
            print(pairs.shape)
            if len(pairs) == 0:
                print("NO NEIGHBORS!!!")
            np.save(folder + "region_pair_list.npy", pairs)


def save_context(args, folder_name_list):
    """final_gen_pair.py:44-70."""
    print("gen context start...")
    for name in folder_name_list:
        folder = _interaction_folder(args, name)
        gen_context(np.load(folder + "region_pair_list.npy"), folder, args)
        for region_folder in _region_folders(folder + "%s_adv_single_region/" % args.mode):
            gen_context(np.load(region_folder + "region_pair_list.npy"), region_folder, args)


def gen_pred_label(model, data, lbl, disturb_fn, save_path, args):
    """final_gen_pair.py:74-88."""
    params = torch.from_numpy(np.load(save_path + "transform_params.npy").astype(np.float32)).to(data.device)
    logits = _dense_logits(model, disturb_fn(data, params).permute(0, 2, 1).contiguous(), args)
    pred = torch.argmax(logits, dim=1)
    with open(save_path + "pred_labels.txt", "w") as f:
        f.write("lbl: %d\npred_lbl: %d\n" % (lbl[0].item(), pred[0].item()))
    np.save(save_path + "pred_labels.npy", np.array([lbl[0].item(), pred[0].item()]))


def save_pred_label(args, disturb_fn, folder_name_list):
    """final_gen_pair.py:90-123."""
    print("saving pred labels...")
    model = load_model(args)
    with torch.no_grad():
        for pc_idx, (data, lbl) in enumerate(data_loader(args)):
            data, lbl = data.to(args.device), lbl.to(args.device)
            folder = _interaction_folder(args, folder_name_list[pc_idx])
            gen_pred_label(model, data, lbl, disturb_fn, folder + "%s_adv/" % args.mode, args)
            for region_folder in _region_folders(folder + "%s_adv_single_region/" % args.mode):
                gen_pred_label(model, data, lbl, disturb_fn, region_folder + "max_pose/", args)
                gen_pred_label(model, data, lbl, disturb_fn, region_folder + "min_pose/", args)


def make_args(argv=None):
    """final_gen_pair.py:323-374, same flags."""
    p = argparse.ArgumentParser(description="Point Cloud Recognition")
    p.add_argument("--model", type=str, default="pointnet", metavar="N",
                   choices=["pointnet", "pointnet2", "pointconv", "dgcnn", "gcnn", "gcnn_adv"])
    p.add_argument("--test_batch_size", type=int, default=1, metavar="batch_size", help="Size of batch)")
    p.add_argument("--dataset", type=str, default="shapenet", metavar="N", choices=["modelnet10", "shapenet"])
    p.add_argument("--no_cuda", type=bool, default=False, help="enables CUDA training")
    p.add_argument("--seed", type=int, default=1, metavar="S", help="random seed (default: 1)")
    p.add_argument("--device_id", type=int, default=0)
    p.add_argument("--mode", default="rotate", type=str)
    p.add_argument("--ratio", default=DEFAULT_RATIOS, type=int)
    p.add_argument("--num_pairs_random", default=300, type=int)
    p.add_argument("--num_save_context_max", default=100, type=int)
    p.add_argument("--softmax_type", default="modified", type=str, choices=["normal", "modified"])
    p.add_argument("--synthetic", action="store_true")
    p.add_argument("--num_clouds", type=int, default=30)
    return p.parse_args(argv)


def run(args):
    """Same stage order as final_gen_pair.py:323-374.  Host RNG streams that run on from cloud to cloud + one small search
    per cloud: never sharded by cloud (the draws of cloud k depend on what clouds < k consumed)."""
    names = get_folder_name_list(args)
    disturb_fn = translate_pc if args.mode == "trans" else rotate_xyz
    save_pair_random(args, names)
    check_adv_success(args, disturb_fn, names)
    save_pair_single_region(args, names)
    save_context(args, names)
    save_pred_label(args, disturb_fn, names)


@iqdist.record
def main(argv=None):
    args = make_args(argv)
    finish_args(args)
    rank0_only(run, args, "pair generation")
