"""final_kernel_shapley.py - region Shapley values by the regression (KernelSHAP) estimator (kernelshap.py; the reference has
none: it only walks sampled permutations, shapley_stage.py).

Per selected cloud, under the experiment folder that ``exp_folder`` derives from ``--num_regions`` (2 to 64, default 32):

    kernelshap/coalitions.npy                     (M,) uint64    the sampled rows, bit r = region r kept
    kernelshap/rewards.npy                        (M,) float32   their rewards
    kernelshap/region_shapley_value.npy           (n,) float64   the estimate from all M rows
    kernelshap/running_counts.npy                 (k,) int64     row counts c (n + 1), c in stage 1's sample counts, <= M
    kernelshap/running_region_shapley_value.npy   (k, n) float64 the estimate from the first count rows
    kernelshap/sampling_error.json                with --compare_exact (at most 24 regions): per count the max and RMS error, in
                                                  reward units, of this estimator and of stage 1's permutation estimate at the same
                                                  number of model evaluations, against exact.shapley of the same cloud; the last row
                                                  is the largest budget both have
    kernelshap/region_interaction.npy             (n, n) float64 with --pairs: the SHAP-IQ estimate of the pairwise Shapley
                                                  interaction index of every pair of regions from the same M rows (kernelshap.pairs;
                                                  symmetric, zero diagonal); with --compare_exact also a "pairs" object in
                                                  sampling_error.json, its max and RMS error over the pairs against the exact index
                                                  (the mean over the orders of exact.interactions, from the same value table)

    kernelshap/region_shapley_se.npy              (n,) float64   with --se and --gram analytic: the standard error of
                                                  region_shapley_value.npy (kernelshap.phi_se)
    kernelshap/region_interaction_se.npy          (n, n) float64 with --se and --pairs: the standard error of every entry of
                                                  region_interaction.npy (kernelshap.pairs_se; symmetric, zero diagonal)

    kernelshap/region_interaction_cv.npy          (n, n) float64 with --pairs and --control shift|regression: the control-variate
                                                  estimate of the same index from the same rows (kernelshap.pairs_cv; DESIGN.md
                                                  5j), beside region_interaction.npy, which is still written
    kernelshap/region_interaction_cv_se.npy       (n, n) float64 its standard error (symmetric, zero diagonal)
    kernelshap/control.json                       {"control", "ridge", "fold_rows", "paired"} of that estimate; with
                                                  --compare_exact sampling_error.json gains "pairs_cv": max error, RMS error, z_rms

    kernelshap/control_pairs.npy                  (K, 2) int32   with --control sparse: the listed pairs of the sparse
                                                  surrogate, the --control_pairs K (default min(3 n, 2080 - n)) nearest pairs of
                                                  FPS centres; control.json is then {"control", "select": "neighbours", "pairs",
                                                  "features", "fold_rows", "ridge", "status"}

Without --pairs, without --se and without --control, every artefact is what it was before the flag existed, byte for byte.
--se is the sampling error of drawn rows: with --samples all, or with the sampled Gram matrix and no --pairs, there is nothing it could write and the
parser says so.  With --compare_exact, sampling_error.json gains "z_rms", the RMS of (estimate - exact) / se - about 1 for a
calibrated bar - for the values whenever region_shapley_se.npy is written, and inside "pairs" for the interactions.

``--samples`` is the number of rows M (model evaluations; default 1000 (n + 1), stage 1's budget; ``all``: the enumerated game).
With --compare_exact both estimates are read off ONE exact value table, not run through the network again; the permutations are
the ones stage 1 would draw at this point of the stream, and the generator is put back afterwards, so the flag does not change
what any cloud draws.  Single process: under several ranks rank 0 does the work and the others wait at the end.
"""
import argparse
import json

import numpy as np
import torch

from . import dist as iqdist
from . import exact, hip_ops, kernelshap
from . import shapley_stage as stage1
from .final_util import NUM_REGIONS, get_folder_name_list, load_model, mkdir


FILES = ("coalitions", "rewards", "region_shapley_value", "running_counts", "running_region_shapley_value")
OPTIONAL = {"interaction": "region_interaction", "phi_se": "region_shapley_se", "interaction_se": "region_interaction_se",
            "interaction_cv": "region_interaction_cv", "interaction_cv_se": "region_interaction_cv_se"}   # a game's key -> file


def artefacts(g):
    """A game of kernelshap.game or wide_kernelshap.game -> dict of one cloud's artefacts: the FILES as ndarrays, v_full, v_empty."""
    running = g["running"]
    return {"coalitions": g["keep"].cpu().numpy().view(np.uint64), "rewards": g["v"].cpu().numpy(), "region_shapley_value": g["phi"],
            "running_counts": np.array(sorted(running), dtype=np.int64),
            "running_region_shapley_value": np.array([running[c] for c in sorted(running)], dtype=np.float64).reshape(len(running), len(g["phi"])),
            "v_full": g["v_full"], "v_empty": g["v_empty"], **{name: g[key] for key, name in OPTIONAL.items() if key in g},
            **({"control": g["control"]} if "control" in g else {})}


def save(folder, out):
    for key in FILES + tuple(name for name in OPTIONAL.values() if name in out):
        np.save(folder + "%s.npy" % key, out[key])
    if "control" in out and "pairs" in out["control"]:           # the sparse control: its list beside what it made of it
        info = out["control"]
        np.save(folder + "control_pairs.npy", info["pairs"])
        with open(folder + "control.json", "w") as f:
            json.dump({"control": info["control"], "select": "neighbours", "pairs": int(len(info["pairs"])),
                       "features": int(info["features"]), "fold_rows": info["fold_rows"], "ridge": info["ridge"],
                       "status": info["status"]}, f)
    elif "control" in out:
        with open(folder + "control.json", "w") as f:
            json.dump({key: out["control"][key] for key in ("control", "ridge", "fold_rows", "paired")}, f)


def add_pairs_flag(parser):
    """--pairs; a namespace parsed without it holds no trace of the flag (``wants_pairs`` reads it)."""
    parser.add_argument("--pairs", action="store_true", default=argparse.SUPPRESS,
                        help="also write kernelshap/region_interaction.npy: the pairwise Shapley interaction index of every pair "
                             "of regions, estimated from the same rows (SHAP-IQ), no further model evaluation")


def wants_pairs(args):
    return bool(getattr(args, "pairs", False))


def add_se_flag(parser):
    """--se; a namespace parsed without it holds no trace of the flag (``wants_se`` reads it)."""
    parser.add_argument("--se", action="store_true", default=argparse.SUPPRESS,
                        help="also write the standard errors of the sampled estimates, from the second moment of the same rows: "
                             "kernelshap/region_shapley_se.npy (analytic Gram matrix) and, with --pairs, region_interaction_se.npy")


def wants_se(args):
    return bool(getattr(args, "se", False))


def check_se(parser, args, gram):
    """--se needs drawn rows and something to put a bar on: a parser error with --samples all, and with the sampled Gram matrix
    unless --pairs is there."""
    if not wants_se(args):
        return
    if args.samples == "all":
        parser.error("--se with --samples all: the enumerated game has no sampling error")
    if gram != "analytic" and not wants_pairs(args):
        parser.error("--se with --gram %s and no --pairs: phi under the sampled Gram matrix has no standard error here "
                     "(--gram analytic, or --pairs)" % gram)


def add_control_flag(parser, choices):
    """--control and --control_pairs; a namespace parsed without one holds no trace of it (``control_of``, ``control_pairs_of``)."""
    parser.add_argument("--control", choices=list(choices) + list(kernelshap.LIST_CONTROLS), default=argparse.SUPPRESS,
                        help="with --pairs: also write kernelshap/region_interaction_cv.npy, its standard error and control.json - the "
                             "control-variate estimate of the all-pairs map from the same rows (shift: the additive game; regression: "
                             "a cross-fitted 2-additive surrogate; sparse: the same with all singles and the --control_pairs nearest "
                             "pairs of regions, 2 to 1024 regions), no further model evaluation; default none")
    parser.add_argument("--control_pairs", type=int, default=argparse.SUPPRESS, metavar="K",
                        help="with --control sparse: the pairs of the surrogate, the K pairs of regions whose FPS centres are "
                             "nearest; default min(3 num_regions, 2080 - num_regions); num_regions + K <= 2080")


def control_of(args):
    return getattr(args, "control", "none")


def control_pairs_of(args):
    """The K of --control sparse: --control_pairs, or kernelshap.default_control_pairs; None for any other control."""
    if control_of(args) not in kernelshap.LIST_CONTROLS:
        return None
    return getattr(args, "control_pairs", kernelshap.default_control_pairs(args.num_regions))


def control_arguments(args, data, fps_index):
    """What a stage hands ``game`` for --control: nothing without the flag; for the sparse control also the count of pairs and the
    FPS centres of the regions ((R,3): point fps_index[r] of the cloud is the centre of region r)."""
    if control_of(args) == "none":
        return {}
    if control_of(args) not in kernelshap.LIST_CONTROLS:
        return {"control": control_of(args)}
    idx = torch.as_tensor(np.asarray(fps_index).reshape(-1)[:args.num_regions].astype(np.int64), device=data.device)
    return {"control": control_of(args), "control_pairs": control_pairs_of(args), "centres": data[0].index_select(0, idx).cpu().numpy()}


def check_control(parser, args):
    """--control other than none needs --pairs and drawn rows: a parser error without --pairs and with --samples all.
    --control_pairs belongs to --control sparse: a parser error without it, below 0 and where num_regions + K exceeds 2080 or K the
    pairs there are."""
    if hasattr(args, "control_pairs"):
        n, k = args.num_regions, args.control_pairs
        if control_of(args) not in kernelshap.LIST_CONTROLS:
            parser.error("--control_pairs without --control sparse: only the sparse surrogate takes a list of pairs")
        if k < 0 or n + k > kernelshap.MAX_SPARSE_FEATURES:
            parser.error("--control_pairs %d: 0 <= K and num_regions + K <= %d" % (k, kernelshap.MAX_SPARSE_FEATURES))
        if k > n * (n - 1) // 2:
            parser.error("--control_pairs %d: %d regions have %d pairs" % (k, n, n * (n - 1) // 2))
    if control_of(args) == "none":
        return
    if not wants_pairs(args):
        parser.error("--control %s without --pairs: the control variate belongs to the all-pairs map" % control_of(args))
    if args.samples == "all":
        parser.error("--control with --samples all: the enumerated game has no sampling error to reduce")


def z_rms(est, exact_value, se):
    """The RMS of (estimate - exact) / se over the entries: about 1 where the bars are calibrated."""
    return float(np.sqrt(np.mean(((np.asarray(est) - exact_value) / se) ** 2)))


def add_sample_flags(parser, enumerated=False):
    """--samples and --unpaired; ``enumerated``: the stage also takes ``--samples all``."""
    parser.add_argument("--samples", type=str if enumerated else int, default=None,
                        help="coalition rows (model evaluations) per cloud; default 1000 (num_regions + 1)"
                             + ("; 'all': every proper coalition" if enumerated else ""))
    parser.add_argument("--unpaired", action="store_true", help="do not follow every sampled coalition with its complement")


def check_samples(parser, args, enumerated=False):
    """--samples as a count of at least 2 (an int afterwards), None, or - ``enumerated`` - 'all'; a parser error otherwise."""
    if args.samples is None or (enumerated and args.samples == "all"):
        return
    if not str(args.samples).isdigit() or int(args.samples) < 2:
        parser.error("--samples %s: a count of at least 2%s" % (args.samples, ", or 'all'" if enumerated else ""))
    args.samples = int(args.samples)


def _errors(est, phi):
    err = np.asarray(est) - phi
    return {"max_abs_error": float(np.abs(err).max()), "rms_error": float(np.sqrt((err ** 2).mean()))}


def exact_pairs(v):
    """The exact pairwise Shapley interaction index off a value table -> (n,n) float64, symmetric, zero diagonal: the mean over
    the orders m = 0 .. n-2 of exact.interactions' context-averaged I_ij^(m)."""
    n = int(v.numel()).bit_length() - 1
    out = np.zeros((n, n))
    pr = hip_ops.all_pairs(n)
    out[pr[:, 0], pr[:, 1]] = out[pr[:, 1], pr[:, 0]] = hip_ops.exact_interactions(v).cpu().numpy().mean(axis=1)
    return out


def compare_exact(model, data, lbl, region_id, keep, args, v=None):
    """-> (exact phi, rows of sampling_error.json): for every sample count c of stage 1 whose c (n + 1) evaluations both
    estimators have, and for the largest number of permutations both have, the errors of the permutation estimate of c
    permutations and of this estimator's first c (n + 1) rows.  ``v``: the cloud's exact value table where the caller has it."""
    n = args.num_regions
    if v is None:
        v = exact.value_table(model, data, lbl, region_id, args)
    phi, _, _ = exact.shapley(model, data, lbl, region_id, args, v=v)
    if args.samples == "all":       # the enumerated rows are no sample: only the final estimate is compared
        return phi, []
    state = np.random.get_state()
    all_orders = stage1.generate_all_orders(None, args, save=False)
    np.random.set_state(state)
    most = min(len(all_orders), keep.numel() // (n + 1))
    budgets = sorted({c for c in stage1.SAMPLE_NUMS if c <= most} | ({most} if most else set()))
    snaps, _ = exact.sampled_from_table(v, all_orders, budgets)
    rows = []
    for c in budgets:
        count = kernelshap.running_counts(n, keep.numel(), not args.unpaired, [c * (n + 1)])[0]
        try:
            est = kernelshap.from_table(v, keep[:count].contiguous(), gram=args.gram)
        except hip_ops.KshapSingular:
            continue
        rows.append({"samples": int(c), "evaluations": int(c * (n + 1)), "permutation": _errors(snaps[c] / c, phi),
                     "kernelshap": dict(rows=int(count), **_errors(est, phi))})
    return phi, rows


def kernel_one_cloud(model, data, lbl, region_id, args, fps_index=None):
    """-> dict of one cloud's artefacts (ndarrays; 'sampling_error' only with --compare_exact, 'region_interaction' only with
    --pairs, 'pairs_error' only with both; with --se the standard errors and, with --compare_exact, 'z_rms' / pairs_error's).
    ``fps_index``: the cloud's FPS centres, read by --control sparse alone."""
    g = kernelshap.game(model, data, lbl, region_id, args, args.samples, not args.unpaired, args.gram, pairs=wants_pairs(args),
                        **({"se": True} if wants_se(args) else {}), **control_arguments(args, data, fps_index))
    out = artefacts(g)
    if args.compare_exact:
        v = exact.value_table(model, data, lbl, region_id, args)
        out["exact"], out["sampling_error"] = compare_exact(model, data, lbl, region_id, g["keep"], args, v)
        if wants_pairs(args):
            upper = np.triu_indices(args.num_regions, 1)
            out["pairs_error"] = _errors(g["interaction"][upper], exact_pairs(v)[upper])
            if "interaction_se" in g:
                out["pairs_error"]["z_rms"] = z_rms(g["interaction"][upper], exact_pairs(v)[upper], g["interaction_se"][upper])
            if "interaction_cv" in g:
                out["pairs_cv_error"] = dict(_errors(g["interaction_cv"][upper], exact_pairs(v)[upper]),
                                             z_rms=z_rms(g["interaction_cv"][upper], exact_pairs(v)[upper],
                                                         g["interaction_cv_se"][upper]))
        if "phi_se" in g:
            out["z_rms"] = z_rms(g["phi"], out["exact"], g["phi_se"])
    return out


def _skip_draw(result_path, args, save=False):
    """What a cloud that is not selected draws: the same sizes and permutations, nothing computed."""
    if args.samples != "all":
        kernelshap.draw(args.num_regions, args.samples or kernelshap.default_samples(args.num_regions), not args.unpaired, args.device)


def run(args):
    model = load_model(args)
    with torch.no_grad():
        for i, name, result_path, data, lbl, fps_index in stage1.selected_clouds(args, get_folder_name_list(args), _skip_draw):
            mkdir(result_path + "kernelshap/")
            region_id = stage1.cal_region_id(data, fps_index, result_path, save=False)
            out = kernel_one_cloud(model, data, lbl, region_id, args, fps_index)
            save(result_path + "kernelshap/", out)
            line = "pointcloud:%s, index:%d, rows:%d, sum(phi)=%.6f, v_full - v_empty=%.6f" % (
                name, i, out["coalitions"].size, out["region_shapley_value"].sum(), out["v_full"] - out["v_empty"])
            if args.compare_exact:
                with open(result_path + "kernelshap/sampling_error.json", "w") as f:
                    json.dump({"num_regions": args.num_regions, "gram": args.gram, "paired": not args.unpaired, "v_full": out["v_full"], "v_empty": out["v_empty"],
                               "final": _errors(out["region_shapley_value"], out["exact"]), "sample_counts": out["sampling_error"],
                               **({"pairs": out["pairs_error"]} if "pairs_error" in out else {}),
                               **({"pairs_cv": out["pairs_cv_error"]} if "pairs_cv_error" in out else {}),
                               **({"z_rms": out["z_rms"]} if "z_rms" in out else {})},
                              f, indent=1)
                if out["sampling_error"]:
                    last = out["sampling_error"][-1]
                    line += ", %d evaluations: rms error %.4g (kernelshap, %s) against %.4g (%d permutations)" % (
                        last["evaluations"], last["kernelshap"]["rms_error"], args.gram, last["permutation"]["rms_error"], last["samples"])
            print(line)


def make_args(argv=None):
    parser = stage1.build_parser()
    add_sample_flags(parser, enumerated=True)
    parser.add_argument("--gram", type=str, default="sampled", choices=list(kernelshap.GRAMS))
    parser.add_argument("--compare_exact", action="store_true",
                        help="also enumerate the game (at most %d regions) and write sampling_error.json" % exact.MAX_PLAYERS)
    add_pairs_flag(parser)
    add_se_flag(parser)
    add_control_flag(parser, kernelshap.CONTROLS)
    args = stage1.parse_game_args(parser, argv, NUM_REGIONS, 2, kernelshap.MAX_REGIONS,
                                  "the regression estimator takes 2 to 64 regions (final_wide_kernel_shapley.py: 65 to 1024)")
    check_samples(parser, args, enumerated=True)
    check_se(parser, args, args.gram)
    check_control(parser, args)
    if (args.compare_exact or args.samples == "all") and args.num_regions > exact.MAX_PLAYERS:
        parser.error("--num_regions %d: --compare_exact and --samples all enumerate 2^num_regions coalitions; at most %d regions"
                     % (args.num_regions, exact.MAX_PLAYERS))
    return args


@iqdist.record
def main(argv=None):
    args = make_args(argv)
    stage1.finish_args(args)
    stage1.rank0_only(run, args, "kernelshap")


if __name__ == "__main__":
    main()
