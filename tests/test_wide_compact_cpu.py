"""CPU: the wide entries of the compact coalition paths are bound, and ``coalitions="compact"`` has no CPU form."""
import argparse

import numpy as np
import pytest
import torch

from interpret_quality_amd import _lib, wide
from interpret_quality_amd.dgcnn import GCNN_cls

NEW = ("iq_dgcnn_coalitions_wide", "iq_pointnet2_coalitions_wide", "iq_pointconv_coalitions_wide",
       "iq_pointconv_coalitions_cached_wide")


def test_the_four_wide_entries_are_bound_with_the_twin_arguments_plus_r():
    for name in NEW:
        assert name in _lib.SIGNATURES
        res, args = _lib.SIGNATURES[name]
        twin_res, twin_args = _lib.SIGNATURES[name[:-len("_wide")]]
        assert res == twin_res and len(args) == len(twin_args) + 1
        assert args[:-2] == twin_args[:-1] and args[-2] == _lib._I and args[-1] == twin_args[-1]    # ..., int R, stream
    lib = _lib.load()
    assert all(hasattr(lib, name) for name in NEW) and lib.iq_version() == _lib.ABI_VERSION >= 108


def test_wide_entries_check_the_region_count_before_anything_else():
    lib = _lib.load()
    for r in (0, 1025):
        calls = (lambda: lib.iq_dgcnn_coalitions_wide(None, None, None, None, None, None, None, None, 0, 0, 1, 64, 0, r, None),
                 lambda: lib.iq_pointnet2_coalitions_wide(None, None, None, None, None, None, None, None, 0, 0, 1, 64, r, None),
                 lambda: lib.iq_pointconv_coalitions_wide(None, None, None, None, None, None, None, None, 0, 0, 1, 64, r, None),
                 lambda: lib.iq_pointconv_coalitions_cached_wide(None, None, None, None, None, None, None, None, 0, 0, 1, 64, None, r,
                                                                 None))
        for call in calls:
            assert call() != 0 and ("R=%d" % r).encode() in lib.iq_last_error()


def _game():
    model = GCNN_cls(argparse.Namespace(dataset="modelnet10", k=20)).eval()
    data = torch.zeros((1, 128, 3))
    rid = np.arange(128)
    args = argparse.Namespace(model="gcnn", softmax_type="modified", num_points=128, num_regions=128, verbose=False)
    return model, data, rid, args


def test_compact_with_a_cpu_tensor_is_an_error():
    model, data, rid, args = _game()
    keep = np.ones((3, 2), dtype=np.uint64)
    orders = np.stack([np.arange(128)])
    with pytest.raises(_lib.IqError):
        wide.coalition_logits(model, data, rid, keep, args, coalitions="compact")
    with pytest.raises(_lib.IqError):
        wide.prefix_logits(model, data, rid, orders, args, coalitions="compact")
    with pytest.raises(_lib.IqError):
        wide.shapley(model, data, torch.zeros((1,), dtype=torch.int64), rid, orders, args, coalitions="compact")
    with pytest.raises(_lib.IqError):
        wide.interaction_logits(model, data, rid, np.array([[0, 1]]), np.zeros((1, 1, 0), dtype=np.int64), args, coalitions="compact")


def test_an_unknown_coalitions_value_is_an_error():
    model, data, rid, args = _game()
    with pytest.raises(_lib.IqError):
        wide.coalition_logits(model, data, rid, np.ones((3, 2), dtype=np.uint64), args, coalitions="fused")


def test_the_drivers_take_the_flag_and_default_to_none():
    from interpret_quality_amd import wide_interaction_stage, wide_stage
    base = ["--model", "gcnn", "--dataset", "modelnet10", "--synthetic"]
    for stage in (wide_stage, wide_interaction_stage):
        assert stage.make_args(base).coalitions is None
        assert stage.make_args(base + ["--coalitions", "compact"]).coalitions == "compact"
        with pytest.raises(SystemExit):
            stage.make_args(base + ["--coalitions", "fast"])
