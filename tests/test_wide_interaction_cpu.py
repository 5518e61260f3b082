"""CPU: the host side of the multi-order interactions of wide games (more than 64 regions) - the (pair, context) keep rows, the
context draws, the driver's argument checks and the new entry point of the C ABI."""
import argparse
import itertools
import os
import re

import numpy as np
import pytest
import torch
from scipy.special import comb

from conftest import REPO
from interpret_quality_amd import _lib, build, gen_pair, interaction, wide, wide_interaction_stage
from oracle import ref_cpu


def _point_flags(keep, rid):
    """(B,W) uint64 keep rows -> (B,N) bool: bit rid[n] of row b."""
    words = keep[:, rid >> 6]
    return ((words >> (rid & 63).astype(np.uint64)) & np.uint64(1)).astype(bool)


def _oracle_flags(rid, pairs, ctx):
    """The keep flags oracle.ref_cpu.interaction_masked_batch applies (its np.isin sets), read off its output: the cloud is
    all ones and the centre all zeros, so an output coordinate is 1.0 exactly where the point is kept."""
    n = rid.shape[0]
    data_cf, center = torch.ones((1, 3, n)), torch.zeros((3,))
    rows = [ref_cpu.interaction_masked_batch(data_cf, center, rid, int(i), int(j), ctx[p]) for p, (i, j) in enumerate(pairs)]
    out = torch.cat(rows, dim=0).numpy()
    assert np.array_equal(out[:, 0], out[:, 1]) and np.array_equal(out[:, 0], out[:, 2]) and np.isin(out, (0.0, 1.0)).all()
    return out[:, 0] == 1.0


def _contexts(rng, pairs, r, c, m):
    rows = []
    for i, j in pairs:
        rest = np.setdiff1d(np.arange(r), [i, j])
        rows.append(np.stack([rng.permutation(rest)[:m] for _ in range(c)]).reshape(c, m))
    return np.stack(rows).astype(np.int64)


@pytest.mark.parametrize("r", [65, 128, 1024])
def test_host_masks_keep_exactly_the_points_the_oracle_keeps(r):
    rng = np.random.default_rng(r)
    n = 1024
    rid = rng.permutation(n) if r == n else rng.integers(0, r, size=n)
    pairs = np.array([[0, r - 1], [63, 64], [r // 2, 5]])
    for m in (0, 1, int((r - 2) * 0.5), r - 2):
        ctx = _contexts(rng, pairs, r, 3, m)
        got = wide.context_keep_masks(pairs, ctx, r)
        assert got.dtype == np.uint64 and got.shape == (4 * 3 * 3, (r + 63) // 64)
        assert np.array_equal(_point_flags(got, rid), _oracle_flags(rid, pairs, ctx)), (r, m)
        valid = np.arange(got.shape[1] * 64) < r
        bits = ((got[:, :, None] >> np.arange(64, dtype=np.uint64)[None, None, :]) & np.uint64(1)).reshape(got.shape[0], -1)
        assert not bits[:, ~valid].any()                                    # no bit at or above R
        assert np.array_equal(bits.sum(axis=1).reshape(-1, 4), np.tile([m + 2, m + 1, m + 1, m], (9, 1)))


@pytest.mark.parametrize("r", [65, 1024])
def test_an_out_of_range_context_entry_is_ignored(r):
    rng = np.random.default_rng(r + 1)
    rid = rng.integers(0, r, size=1024)
    pairs = np.array([[1, r - 2], [64, 3]])
    ctx = _contexts(rng, pairs, r, 2, 9)
    ctx[0, 1, 4], ctx[1, 0, 0], ctx[1, 1, 8] = r, -1, r + 70             # no point carries such a region id
    got = wide.context_keep_masks(pairs, ctx, r)
    assert np.array_equal(_point_flags(got, rid), _oracle_flags(rid, pairs, ctx))
    clean = ctx.copy()
    clean[0, 1, 4], clean[1, 0, 0], clean[1, 1, 8] = ctx[0, 1, 0], ctx[1, 0, 1], ctx[1, 1, 0]   # a repeated entry adds nothing
    assert np.array_equal(got, wide.context_keep_masks(pairs, clean, r))


@pytest.mark.parametrize("r,m", [(64, 0), (64, 31), (64, 62), (32, 15), (2, 0)])
def test_host_masks_equal_the_narrow_path_up_to_64_regions(r, m):
    rng = np.random.default_rng(10 * r + m)
    pairs = np.array([[0, r - 1], [r - 1, r // 2]])
    ctx = _contexts(rng, pairs, r, 5, m)
    got = wide.context_keep_masks(pairs, ctx, r)
    assert got.shape == (40, 1) and np.array_equal(got[:, 0], interaction.context_keep_masks(pairs, ctx, r))


def test_bad_shapes_and_region_counts_are_refused():
    pairs = np.array([[0, 1]])
    with pytest.raises(_lib.IqError):
        wide.context_keep_masks(pairs, np.zeros((2, 1, 3), dtype=np.int64), 128)       # two context rows for one pair
    with pytest.raises(_lib.IqError):
        wide.context_keep_masks(pairs, np.zeros((1, 3), dtype=np.int64), 128)
    with pytest.raises(_lib.IqError):
        wide.context_keep_masks(pairs, np.zeros((1, 1, 3), dtype=np.int64), 1025)
    with pytest.raises(_lib.IqError):
        wide.gen_context(pairs, 1025, [0.5], 3)


def _reference_gen_context(pairs, num_regions, ratios, num_save_context_max):
    """final_gen_pair.py:18-43 written out: np.random.choice on a python list, np.array over the per-pair lists."""
    out = []
    for ratio in ratios:
        context_list = []
        m = int((num_regions - 2) * ratio)
        for region_i, region_j in pairs:
            all_s = list(range(num_regions))
            all_s.remove(region_i)
            all_s.remove(region_j)
            if comb(len(all_s), m) > num_save_context_max:
                context_this_pair = [np.random.choice(all_s, m, replace=False) for _ in range(num_save_context_max)]
            else:
                context_this_pair = list(itertools.combinations(all_s, m))
            context_list.append(context_this_pair)
        out.append(np.array(context_list))
    return out


def test_context_draws_are_the_reference_loop():
    r, cmax = 70, 70
    ratios = [0., 0.02, 0.1, 0.5, 0.99, 1.]          # m = 0, 1 (all 68 combinations listed), 6, 34, 67 (68 listed), 68
    np.random.seed(11)
    pairs = gen_pair.gen_pair_random(argparse.Namespace(num_regions=r, num_pairs_random=4))
    np.random.seed(12)
    want = _reference_gen_context(pairs.tolist(), r, ratios, cmax)
    state_want = np.random.get_state()
    after_want = np.random.random()
    np.random.seed(12)
    got = wide.gen_context(pairs, r, ratios, cmax)
    state_got = np.random.get_state()
    assert [w.shape for w in want] == [(4, 1, 0), (4, 68, 1), (4, 70, 6), (4, 70, 34), (4, 68, 67), (4, 1, 68)]
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.shape == w.shape and g.dtype == np.int64 and np.array_equal(g, w)
    assert state_got[0] == state_want[0] and np.array_equal(state_got[1], state_want[1]) and state_got[2:] == state_want[2:]
    assert np.random.random() == after_want
    # the narrow int16 form the driver saves: the same draws, the same numbers
    np.random.seed(12)
    small = list(wide.iter_contexts(pairs, r, ratios, cmax, dtype=np.int16))
    assert all(s.dtype == np.int16 and np.array_equal(s, w) for s, w in zip(small, want))
    # every context avoids its pair and names m distinct regions
    for g in got:
        for p, (i, j) in enumerate(pairs):
            assert not np.isin(g[p], [i, j]).any()
            assert all(len(set(row)) == g.shape[2] for row in g[p].tolist())


def test_reused_stages_are_the_narrow_functions():
    assert wide.gen_pair_random is gen_pair.gen_pair_random and wide.interactions is interaction.compute_order_interaction


def test_driver_refuses_region_counts_outside_its_range():
    for bad in ("64", "1025"):
        with pytest.raises(SystemExit):
            wide_interaction_stage.make_args(["--model", "pointnet", "--num_regions", bad])
    args = wide_interaction_stage.make_args(["--model", "pointnet", "--num_regions", "1024", "--transform_params", "x.npy"])
    assert args.num_regions == 1024 and args.transform_params == "x.npy" and args.device_id == 0
    assert args.num_pairs_random == 300 and args.num_save_context_max == 100 and args.gen_pair_seed == 1
    assert args.softmax_type == "modified" and args.output_type == "pred" and args.mode == "rotate"
    assert wide_interaction_stage.CONTEXT_DTYPE == np.int16 and np.iinfo(np.int16).max >= wide.MAX_REGIONS


def test_entry_point_is_declared_exported_and_versioned():
    header = open(os.path.join(REPO, "include", "iq.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"\bint\s+iq_context_keep_masks_wide\s*\(", code)
    build.build(verbose=False)
    lib = _lib.load()
    assert hasattr(lib, "iq_context_keep_masks_wide") and "iq_context_keep_masks_wide" in _lib.SIGNATURES
    version = int(re.search(r"#define IQ_ABI_VERSION (\d+)", header).group(1))
    assert _lib.ABI_VERSION == lib.iq_version() == version >= 106
