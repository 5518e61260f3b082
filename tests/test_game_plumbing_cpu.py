"""CPU: the single copies of the host-side game plumbing that the narrow, wide and exact paths share - the region-word builder
behind the four host mask builders, the per-cloud driver loop and the host context generator."""
import argparse
import itertools

import numpy as np
import pytest
import torch
from scipy.special import comb

from interpret_quality_amd import final_common, gen_pair, hip_ops, interaction, shapley_stage, wide, wide_stage
from interpret_quality_amd._lib import IqError
from interpret_quality_amd.final_util import set_random


def _words_bit_by_bit(ids, r):
    """The set of the ids that lie in [0, R), one bit at a time on python integers -> (W,) uint64."""
    words = [0] * ((r + 63) // 64)
    for i in ids:
        if 0 <= int(i) < r:
            words[int(i) // 64] |= 1 << (int(i) % 64)
    return np.array(words, dtype=np.uint64)


def _id_rows(r):
    """(k, rows of k ids): k = 0, 1, R valid ids, then rows with -1 and R among valid ids and with a repeated id."""
    rng = np.random.default_rng(r)
    yield np.zeros((2, 0), dtype=np.int64)
    yield np.array([[0], [r - 1]])
    yield np.stack([rng.permutation(r), np.arange(r)])
    yield np.array([[r - 1, -1, 0, r, r // 2], [r, r, -1, r - 1, r + 63], [r // 2, 0, r // 2, -1, r // 2]])


@pytest.mark.parametrize("r", [1, 63, 64, 65, 128, 1024])
def test_region_words_equal_a_bit_by_bit_loop(r):
    for ids in _id_rows(r):
        got = hip_ops.region_words(ids, r)
        assert got.dtype == np.uint64 and got.shape == (ids.shape[0], (r + 63) // 64)
        for row, g in zip(ids, got):
            assert np.array_equal(g, _words_bit_by_bit(row, r))
        pref = hip_ops.region_words(ids, r, prefixes=True)
        assert pref.dtype == np.uint64 and pref.shape == (ids.shape[0], ids.shape[1] + 1, (r + 63) // 64)
        for row, p in zip(ids, pref):
            for i in range(ids.shape[1] + 1):
                assert np.array_equal(p[i], _words_bit_by_bit(row[:i], r))
    lead = np.arange(12).reshape(2, 3, 2) % r                     # any leading shape
    assert np.array_equal(hip_ops.region_words(lead, r).reshape(6, -1), hip_ops.region_words(lead.reshape(6, 2), r))


@pytest.mark.parametrize("r", [1, 2, 32, 63, 64])
def test_narrow_builders_give_one_word_and_still_reject_an_id_outside_the_game(r):
    rng = np.random.default_rng(r)
    orders = np.stack([rng.permutation(r) for _ in range(3)])
    keep = final_common.prefix_keep_masks(orders, r)
    assert keep.dtype == np.uint64 and keep.shape == (3 * (r + 1),)
    want = [sum(1 << int(x) for x in orders[o][:i]) for o in range(3) for i in range(r + 1)]
    assert keep.tolist() == want
    pairs = np.array([[0, r - 1], [r - 1, r // 2]])
    ctx = rng.integers(0, r, size=(2, 3, 4))
    k = interaction.context_keep_masks(pairs, ctx, r)
    assert k.dtype == np.uint64 and k.shape == (2 * 3 * 4,)
    for p, (i, j) in enumerate(pairs):
        for c in range(3):
            s = sum(1 << int(x) for x in set(ctx[p, c].tolist()))
            assert k.reshape(2, 3, 4)[p, c].tolist() == [s | 1 << int(i) | 1 << int(j), s | 1 << int(i), s | 1 << int(j), s]
    bad = orders.copy()
    bad[1, 0] = r
    with pytest.raises(IqError, match="orders: index at position"):
        final_common.prefix_keep_masks(bad, r)
    with pytest.raises(IqError, match="region_pair_list: index at position"):
        interaction.context_keep_masks(np.array([[0, r]]), ctx[:1], r)
    ctx[1, 2, 3] = r
    with pytest.raises(IqError, match="context_list: index at position"):
        interaction.context_keep_masks(pairs, ctx, r)


@pytest.mark.parametrize("r", [65, 128])
def test_wide_builders_ignore_what_the_narrow_ones_reject(r):
    orders = np.array([np.r_[np.arange(r - 2), [r, -1]]])
    got = wide.prefix_keep_masks(orders, r)
    assert got.shape == (r + 1, (r + 63) // 64)
    assert np.array_equal(got[r - 2], got[r]) and np.array_equal(got[r], _words_bit_by_bit(np.arange(r - 2), r))
    k = wide.context_keep_masks(np.array([[1, r]]), np.array([[[-1, 64, r + 1]]]), r)
    assert [row.tolist() for row in k] == [_words_bit_by_bit(x, r).tolist() for x in ([1, 64], [1, 64], [64], [64])]


class _Loader:
    """4 clouds; records which ones the loop reached."""

    def __init__(self):
        self.reached = []

    def __iter__(self):
        for i in range(4):
            self.reached.append(i)
            yield torch.full((1, 8, 3), float(i)), torch.tensor([i])


def _loop_args(tmp_path, subset):
    args = argparse.Namespace(dataset="shapenet", num_points=8, num_regions=65, num_samples_save=3, device=torch.device("cpu"),
                              exp_folder=str(tmp_path) + "/exp/", cloud_subset=subset)
    return args, ["cloud%d" % i for i in range(4)]


@pytest.mark.parametrize("subset", [{2}, None])
def test_cloud_loop_draws_for_skipped_clouds_and_stops_after_the_last_selected_one(tmp_path, monkeypatch, subset):
    monkeypatch.chdir(tmp_path)
    args, names = _loop_args(tmp_path, subset)
    fps = np.arange(4 * 65).reshape(4, 65)
    np.save(shapley_stage.fps_index_path(args), fps)
    drawn = []

    def draw(result_path, a, save=True):
        assert a is args and save is False
        drawn.append(result_path)
        return wide_stage.generate_all_orders(result_path, a, save=save)

    loader = _Loader()
    set_random(3)
    seen = []
    for i, name, result_path, data, lbl, fps_index in shapley_stage.selected_clouds(args, names, draw, loader):
        assert name == names[i] and result_path == args.exp_folder + name + "/" and (tmp_path / "exp" / name).is_dir()
        assert float(data[0, 0, 0]) == i and int(lbl[0]) == i and np.array_equal(fps_index, fps[i])
        seen.append((i, wide_stage.generate_all_orders(result_path, args, save=False)))   # what a driver draws for its cloud
    state = np.random.get_state()
    # the hand-written sequence: every cloud up to the last selected one draws its permutations, selected or not
    set_random(3)
    last = 2 if subset else 3
    want = [wide_stage.generate_all_orders("unused/", args, save=False) for _ in range(last + 1)]
    want_state = np.random.get_state()
    assert state[0] == want_state[0] and np.array_equal(state[1], want_state[1]) and state[2:] == want_state[2:]
    if subset:
        assert drawn == [args.exp_folder + "cloud0/", args.exp_folder + "cloud1/"] and [i for i, _ in seen] == [2]
        assert loader.reached == [0, 1, 2, 3]      # cloud 3 is what ends the loop: fetched, never drawn for, moved or yielded
        assert not (tmp_path / "exp" / "cloud0").exists() and not (tmp_path / "exp" / "cloud3").exists()
    else:
        assert drawn == [] and [i for i, _ in seen] == [0, 1, 2, 3]
    for i, orders in seen:
        assert orders.shape == (3, 65) and np.array_equal(orders, want[i])


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


@pytest.mark.parametrize("cmax,pairs", [(3, [[0, 5], [4, 2]]), (100, [[0, 5], [4, 2]]), (3, [])])
def test_host_gen_context_writes_the_reference_loops_files(tmp_path, cmax, pairs):
    """Without a device gen_pair.gen_context is the reference's host loop: the files, their dtypes (np.array's own choice: int64,
    float64 for the empty context of ratio 0 and for no pairs at all) and the generator state after it."""
    ratios = [0., 0.5, 1.]
    args = argparse.Namespace(num_regions=6, num_save_context_max=cmax, ratio=ratios)
    np.random.seed(21)
    want = _reference_gen_context(pairs, 6, ratios, cmax)
    want_state = np.random.get_state()
    np.random.seed(21)
    gen_pair.gen_context(np.array(pairs), str(tmp_path) + "/", args)
    state = np.random.get_state()
    assert state[0] == want_state[0] and np.array_equal(state[1], want_state[1]) and state[2:] == want_state[2:]
    if pairs:
        assert [w.shape for w in want] == [(2, 1, 0), (2, 3 if cmax == 3 else 6, 2), (2, 1, 4)]
        assert [w.dtype for w in want] == [np.float64, np.int64, np.int64]
    else:
        assert [w.shape for w in want] == [(0,)] * 3
    for ratio, w in zip(ratios, want):
        got = np.load(str(tmp_path) + "/ratio%d_context_list.npy" % int(ratio * 100))
        assert got.shape == w.shape and got.dtype == w.dtype and np.array_equal(got, w)
    if pairs:       # the wide generator is the same loop with a chosen dtype
        np.random.seed(21)
        for g, w in zip(wide.gen_context(pairs, 6, ratios, cmax), want):
            assert g.dtype == np.int64 and g.shape == w.shape and np.array_equal(g, w)
