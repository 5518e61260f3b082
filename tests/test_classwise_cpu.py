"""All-class games without a GPU: the two entry points are declared, bound and versioned; the NumPy restatement of both
(tests/classwise_ref.py) agrees with the oracle's single-label reward and sampling loop per label; the driver's refusals."""
import argparse
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO
import classwise_ref
from interpret_quality_amd import _lib, class_stage

ENTRIES = ("iq_reward_classes", "iq_shapley_accum_games", "iq_shapley_games_scratch_bytes")


def test_entries_are_declared_bound_and_versioned():
    header = open(os.path.join(REPO, "include", "iq.h")).read()
    declared = set(re.findall(r"\b(iq_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    for name in ENTRIES:
        assert name in declared, name
        assert name in _lib.SIGNATURES, name
    version = int(re.search(r"#define IQ_ABI_VERSION (\d+)", header).group(1))
    assert _lib.ABI_VERSION == _lib.load().iq_version() == version >= 118


def test_scratch_does_not_depend_on_the_game_count():
    lib = _lib.load()
    for r, s in ((1, 1), (32, 1000), (1024, 1000)):
        sizes = {lib.iq_shapley_games_scratch_bytes(r, s, g) for g in (1, 40, 65535)}
        assert len(sizes) == 1 and min(sizes) >= 2 * r * s
    for r, s, g in ((0, 1, 1), (1025, 1, 1), (4, -1, 1), (4, 1, 0), (4, 1, 65536)):
        assert lib.iq_shapley_games_scratch_bytes(r, s, g) == 0


# ---- a tiny game: R = 4 regions of one point each, S = 3 permutations, a random C = 5 logit table standing in for the model ----
R, S, C = 4, 3, 5


class TableModel:
    """The 'network': a coalition's logits are a row of a random (2^R, C) table, looked up by which points kept their place."""

    def __init__(self, data, table):
        self.data, self.table = data, table

    def __call__(self, x):                              # x (B,3,N), as cal_reward hands it over
        kept = (x.permute(0, 2, 1) == self.data).all(dim=2)              # (B,N)
        mask = (kept.long() << torch.arange(kept.shape[1])).sum(dim=1)
        return self.table[mask], None


@pytest.fixture(scope="module")
def tiny():
    rng = np.random.RandomState(7)
    data = torch.from_numpy(rng.randn(1, R, 3).astype(np.float32))
    table = torch.from_numpy((4.0 * rng.randn(1 << R, C)).astype(np.float32))
    orders = np.stack([rng.permutation(R) for _ in range(S)])
    region_id = np.arange(R)
    # the logits of the prefix coalitions in the reference's row order
    keep = np.array([[sum(1 << int(r) for r in o[:i]) for i in range(R + 1)] for o in orders]).reshape(-1)
    return TableModel(data, table), data, region_id, orders, table[torch.from_numpy(keep)]


@pytest.mark.parametrize("softmax_type", ["modified", "normal"])
def test_restatement_against_the_oracle_per_label(tiny, softmax_type):
    from oracle import ref_cpu
    model, data, region_id, orders, logits = tiny
    modified = softmax_type == "modified"
    v = classwise_ref.reward_classes(logits.numpy(), None, modified)
    assert v.shape == (C, S * (R + 1)) and v.dtype == np.float32
    total, snaps = classwise_ref.shapley_accum_games(v, orders, (1, S))
    for label in range(C):
        want_v = ref_cpu.get_reward(logits, torch.tensor([label]), softmax_type).numpy()
        np.testing.assert_allclose(v[label], want_v, rtol=2e-6, atol=2e-6)      # the bar of tests/test_hip_parity.py::test_reward
        want_total, want_rows = ref_cpu.shap_sampling_stage1(model, data, torch.tensor([label]), region_id, orders, R, softmax_type)
        # the oracle's rewards differ from the restatement's in the last bits (another logsumexp): R differences of them per region
        bar = 4 * S * 2e-6 * (1 + np.abs(want_v).max())
        np.testing.assert_allclose(total[label], want_total, rtol=0, atol=bar)
        np.testing.assert_allclose(snaps[label, 0], want_rows[0], rtol=0, atol=bar)
        np.testing.assert_allclose(snaps[label, 1], want_total, rtol=0, atol=bar)
    # a subset with a repeat, unsorted: rows are the single-label rows
    sub = classwise_ref.reward_classes(logits.numpy(), [3, 0, 3], modified)
    assert np.array_equal(sub.view(np.int32), v[[3, 0, 3]].view(np.int32))


@pytest.mark.parametrize("modified", [True, False])
def test_efficiency_per_class(tiny, modified):
    _, _, _, orders, logits = tiny
    v = classwise_ref.reward_classes(logits.numpy(), None, modified)
    total, _ = classwise_ref.shapley_accum_games(v, orders)
    rows = v.astype(np.float64).reshape(C, S, R + 1)
    telescoped = (rows[:, :, -1] - rows[:, :, 0]).sum(axis=1)
    bound = S * R * 2.0 ** -23 * np.abs(v).max(axis=1)       # the float32 rounding of each difference; nothing else is lost
    assert (np.abs(total.sum(axis=1) - telescoped) <= bound).all(), (total.sum(axis=1) - telescoped, bound)


def test_restatement_special_rows():
    z = np.array([[-np.inf, 1.0, -np.inf], [2.0, 2.0, 2.0], [80.0, -80.0, 0.0], [-np.inf, -np.inf, 3.0]], dtype=np.float32)
    v = classwise_ref.reward_classes(z, None, True)
    assert v[1, 0] == np.inf                       # every other logit is -inf: the maximum is not subtracted, log(0) = -inf
    assert v[0, 1] == np.float32(2.0 - (np.log(np.float32(2.0)) + np.float32(2.0)))
    assert np.isfinite(v[:, 2]).all()


# ---- the driver's refusals ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("argv", [["--classes", "x"], ["--classes", "1,,2"], ["--classes", "-1"], ["--classes", ""],
                                  ["--num_regions", "1"], ["--num_regions", "1025"], ["--num_regions", "8", "--route", "keep"],
                                  ["--num_samples", "0"], ["--estimator", "exact"]])
def test_parser_refusals(argv, capsys):
    with pytest.raises(SystemExit) as e:
        class_stage.make_args(["--synthetic"] + argv)
    assert e.value.code == 2
    assert "usage" in capsys.readouterr().err


def test_parser_accepts_classes():
    assert class_stage.make_args(["--classes", "all"]).class_list is None
    assert class_stage.make_args(["--classes", "7,0,7", "--num_regions", "1024"]).class_list == [7, 0, 7]
    assert class_stage.parse_classes("3") == [3]


@pytest.mark.parametrize("regions, script", [(8, "final_shapley_value.py"), (128, "final_wide_shapley.py")])
def test_missing_stage1_file_names_the_stage(tmp_path, regions, script):
    base = str(tmp_path) + "/"
    args = argparse.Namespace(num_regions=regions, estimator="permutation", num_samples=2)
    with pytest.raises(SystemExit) as e:
        class_stage.cloud_files(base, args)
    assert "region_id.npy" in str(e.value) and script in str(e.value)
    np.save(base + "region_id.npy", np.zeros(4, dtype=np.int64))
    with pytest.raises(SystemExit) as e:
        class_stage.cloud_files(base, args)
    assert "all_orders.npy" in str(e.value) and script in str(e.value)
    args.estimator = "kernel"
    region_id, orders = class_stage.cloud_files(base, args)
    assert orders is None and region_id.shape == (4,)
