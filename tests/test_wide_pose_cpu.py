"""CPU: the surface of the wide pose and smoothness stages - iq_smoothness_enum_wide is declared, exported, bound and versioned
(ABI 110); the new drivers' parsers and their checks of stage 1's files.  What the stages compute: tests/test_wide_pose_gpu.py,
tests/test_wide_smoothness_gpu.py."""
import argparse
import os
import re

import numpy as np
import pytest

from interpret_quality_amd import _lib, build, hip_ops, wide, wide_interaction_stage, wide_pose_stage, wide_smoothness_stage

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "iq_smoothness_enum_wide"


def _header():
    return open(os.path.join(REPO, "include", "iq.h")).read()


def _params(entry):
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % entry, code)
    assert m, "%s is not declared in include/iq.h" % entry
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_abi_version_is_at_least_110_on_all_three_sides_and_the_entry_is_bound():
    build.build(verbose=False)
    version = int(re.search(r"#define IQ_ABI_VERSION (\d+)", _header()).group(1))
    lib = _lib.load()
    assert _lib.ABI_VERSION == lib.iq_version() == version >= 110
    assert hasattr(lib, ENTRY) and ENTRY in _lib.SIGNATURES
    assert _params(ENTRY) == _params("iq_smoothness_enum")                    # the same arguments
    assert _lib.SIGNATURES[ENTRY] == _lib.SIGNATURES["iq_smoothness_enum"]
    assert len(getattr(lib, ENTRY).argtypes) == len(_params(ENTRY))
    assert "have no wide form" not in re.sub(r"\s*\n \*\s*", " ", _header())


def test_wide_wrapper_checks_the_region_count_and_the_point_count_before_any_device_work():
    class Cloud:                      # only the shape is looked at before the checks fail
        shape = (2048, 3)
    with pytest.raises(_lib.IqError, match="1025"):
        hip_ops.smoothness_enum_wide(Cloud(), None, 1025, "planarity", "inc")
    with pytest.raises(_lib.IqError, match="N=2048"):
        hip_ops.smoothness_enum_wide(Cloud(), None, 128, "planarity", "inc")
    assert hip_ops.MAX_SMOOTHNESS_POINTS == 1024


@pytest.mark.parametrize("make_args,extra", [(wide_pose_stage.make_args, ["--mode", "scale"]), (wide_smoothness_stage.make_args, [])])
def test_new_parsers_take_65_to_1024_regions(make_args, extra, capsys):
    base = ["--model", "pointnet"] + extra
    args = make_args(base)
    assert args.num_regions == 128 and args.num_samples == 100 and args.route is None and args.coalitions is None
    assert make_args(base + ["--num_regions", "65", "--num_samples", "4", "--route", "keep"]).num_samples == 4
    assert make_args(base + ["--num_regions", "1024"]).num_regions == 1024
    for bad in ("64", "1025"):
        with pytest.raises(SystemExit):
            make_args(base + ["--num_regions", bad])
        assert "the wide stage takes 65 .. 1024 regions" in capsys.readouterr().err


def test_pose_parser_needs_a_mode():
    with pytest.raises(SystemExit):
        wide_pose_stage.make_args(["--model", "pointnet"])
    with pytest.raises(SystemExit):
        wide_pose_stage.make_args(["--model", "pointnet", "--mode", "linearity"])
    assert sorted(wide_pose_stage.MODES) == ["rotate", "scale", "trans"]


def test_adv_pose_sweep_excludes_transform_params(capsys):
    assert wide_interaction_stage.make_args(["--adv_pose", "sweep"]).adv_pose == "sweep"
    assert wide_interaction_stage.make_args([]).adv_pose is None
    with pytest.raises(SystemExit):
        wide_interaction_stage.make_args(["--adv_pose", "sweep", "--transform_params", "x.npy"])
    assert "--transform_params" in capsys.readouterr().err


def test_num_samples_beyond_the_saved_permutations_is_an_error(tmp_path):
    base = str(tmp_path) + "/"
    np.save(base + "all_orders.npy", np.stack([np.random.default_rng(k).permutation(65) for k in range(4)]))
    assert wide_pose_stage.load_orders(base, argparse.Namespace(num_samples=3)).shape == (3, 65)
    assert wide_pose_stage.load_orders(base, argparse.Namespace(num_samples=4)).shape == (4, 65)
    with pytest.raises(SystemExit, match="--num_samples 5 exceeds the 4 permutations"):
        wide_pose_stage.load_orders(base, argparse.Namespace(num_samples=5))


def test_missing_stage_one_artefacts_end_with_the_interaction_stages_message(tmp_path):
    args = argparse.Namespace(exp_folder=str(tmp_path) + "/", num_regions=65)
    with pytest.raises(SystemExit, match="region_id.npy not found: run final_wide_shapley.py --num_regions 65 first"):
        wide_pose_stage.selected_folders(args, ["cloud_a"])
    os.makedirs(tmp_path / "cloud_a")
    np.save(tmp_path / "cloud_a" / "region_id.npy", np.zeros(4))
    with pytest.raises(SystemExit, match="all_orders.npy not found"):
        wide_pose_stage.selected_folders(args, ["cloud_a"])
    np.save(tmp_path / "cloud_a" / "all_orders.npy", np.zeros((1, 4)))
    assert wide_pose_stage.selected_folders(args, ["cloud_a"]) == [(0, str(tmp_path) + "/cloud_a/")]


def test_shapley_over_poses_refuses_an_unknown_route_before_touching_a_device():
    with pytest.raises(_lib.IqError, match="route"):
        wide.shapley_over_poses(None, None, None, None, None, None, route="nonsense")
