"""CPU: the host side of the wide games (more than 64 regions) - the prefix keep rows, the driver's permutation stream and the
constants shared with the header."""
import argparse
import os
import re

import numpy as np
import pytest

from conftest import REPO
from interpret_quality_amd import final_common, hip_ops, wide, wide_stage
from interpret_quality_amd.final_util import set_random
from oracle import ref_cpu


def _prefix_ref(orders, r):
    """Row o*(R+1)+i as a boolean membership vector of orders[o][:i] (np.isin), packed 64 regions to a word, bit r & 63."""
    s = orders.shape[0]
    w = (r + 63) // 64
    out = np.zeros((s * (r + 1), w), dtype=np.uint64)
    regions = np.arange(w * 64)
    weights = np.left_shift(np.uint64(1), (regions & 63).astype(np.uint64)).reshape(w, 64)
    for o in range(s):
        for i in range(r + 1):
            member = np.isin(regions, orders[o, :i]).reshape(w, 64)
            out[o * (r + 1) + i] = np.where(member, weights, np.uint64(0)).sum(axis=1, dtype=np.uint64)
    return out


@pytest.mark.parametrize("r", [1, 64, 65, 128, 200, 1024])
def test_prefix_keep_masks_match_the_isin_restatement(r):
    rng = np.random.default_rng(r)
    s = 3 if r < 1024 else 2
    orders = np.stack([rng.permutation(r) for _ in range(s)])
    got = wide.prefix_keep_masks(orders, r)
    assert got.dtype == np.uint64 and got.shape == (s * (r + 1), (r + 63) // 64)
    assert np.array_equal(got, _prefix_ref(orders, r))
    if r <= 64:
        assert np.array_equal(got[:, 0], final_common.prefix_keep_masks(orders, r))


def test_an_out_of_range_entry_is_ignored_and_bad_shapes_are_refused():
    orders = np.array([[3, 70, 500, 0, 1]])           # 500 and 70 are outside [0, 5)
    got = wide.prefix_keep_masks(orders, 5)
    assert got[:, 0].tolist() == [0, 8, 8, 8, 9, 11]
    with pytest.raises(Exception):
        wide.prefix_keep_masks(np.zeros((2, 4), dtype=np.int64), 5)
    with pytest.raises(Exception):
        wide.prefix_keep_masks(np.zeros((1, 1025), dtype=np.int64), 1025)


def test_driver_permutations_are_the_reference_stream():
    args = argparse.Namespace(num_regions=128, num_samples_save=7)
    set_random(5)
    got = wide_stage.generate_all_orders("unused/", args, save=False)
    set_random(5)
    want = ref_cpu.generate_all_orders(7, 128)
    assert got.shape == (7, 128) and np.array_equal(got, want)
    # the stream runs on: a second cloud's permutations are the reference's next draws
    set_random(5)
    two = ref_cpu.generate_all_orders(14, 128)
    set_random(5)
    wide_stage.generate_all_orders("unused/", args, save=False)
    assert np.array_equal(wide_stage.generate_all_orders("unused/", args, save=False), two[7:])


def test_header_constant_equals_the_python_constant():
    m = re.search(r"#define IQ_MAX_WIDE_REGIONS (\d+)", open(os.path.join(REPO, "include", "iq.h")).read())
    assert m and int(m.group(1)) == hip_ops.MAX_WIDE_REGIONS == wide.MAX_REGIONS == 1024


def test_driver_refuses_region_counts_outside_its_range():
    for bad in ("64", "1025"):
        with pytest.raises(SystemExit):
            wide_stage.make_args(["--model", "pointnet", "--num_regions", bad])
    assert wide_stage.make_args(["--model", "pointnet", "--num_regions", "1024"]).num_regions == 1024


def test_oracle_masking_and_region_ids_do_not_depend_on_the_region_count():
    """oracle.ref_cpu at R = 128: shapley_masked_batch against the np.isin statement of tools/final_common.py:56-60, cal_region_id
    against a float64 nearest-centre search (ids may differ only where two centres are within float32 rounding)."""
    import torch
    from interpret_quality_amd import synth
    pts, _ = synth.make_cloud(3)
    data = torch.from_numpy(pts)[None]
    fps = ref_cpu.farthest_point_sample(data, 128)[0].numpy()
    rid = ref_cpu.cal_region_id(data, fps)
    assert rid.shape == (1024,) and rid.min() == 0 and rid.max() == 127
    d64 = ((pts[:, None, :].astype(np.float64) - pts[fps][None].astype(np.float64)) ** 2).sum(-1)
    best = d64.min(axis=1)
    assert np.all(d64[np.arange(1024), rid] <= best + 1e-5)
    order = np.random.default_rng(0).permutation(128)[None]
    center = data.mean(dim=1).squeeze()
    masked = ref_cpu.shapley_masked_batch(data, center, order, rid).numpy()
    for i in (0, 1, 64, 65, 128):
        keep = np.isin(rid, order[0, :i])
        assert np.array_equal(masked[i], np.where(keep[:, None], pts, center.numpy()[None]))
