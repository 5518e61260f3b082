"""GPU: the device sampler in the stages of a wide game - wide.gen_context with a device against the host loop (arrays, dtypes and
NumPy's global generator afterwards), iq_context_regions_wide against rest[...], and the two drivers that draw,
final_wide_shapley.py and final_wide_interaction.py, with ``--sampler device`` against ``--sampler host``: every file byte for byte."""
import filecmp
import gc
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from interpret_quality_amd import _lib, hip_ops, wide
from interpret_quality_amd.interaction import DEFAULT_RATIOS

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


# ---- 1. contexts ----

MIXED = [0.0, 0.3, 0.02, 0.5, 0.99, 0.04, 1.0]     # at R = 65: m = 0, 18, 1, 31, 62, 2, 63


@pytest.mark.parametrize("r,cmax,ratios", [(65, 100, MIXED), (65, 100, DEFAULT_RATIOS), (128, 5, DEFAULT_RATIOS), (1024, 5, DEFAULT_RATIOS)])
def test_gen_context_on_the_device_equals_the_host_loop(r, cmax, ratios):
    """R = 65 with 100 contexts per pair: C(63, 1) = C(63, 62) = 63 <= 100, so in MIXED m = 1 and m = 62 are enumerated between
    sampled ratios (the default ratios give no such m: only their first and last are enumerated).  R = 128 and 1024 with 5: all
    thirteen ratios."""
    rng = np.random.default_rng(r)
    pairs = np.stack([rng.choice(r, size=2, replace=False) for _ in range(3)])
    pairs[0] = (r - 1, 0)
    np.random.seed(r)
    np.random.standard_normal()                  # a cached Gaussian travels through the device draw untouched
    before = np.random.get_state()
    want = wide.gen_context(pairs, r, ratios, cmax)
    want_state = np.random.get_state()
    enumerated = [w.shape[1] for w in want if w.shape[1] != cmax]
    assert enumerated == ([1, 63, 63, 1] if ratios is MIXED else [1, 1]) and len(want) == len(ratios)
    np.random.set_state(before)
    got = wide.gen_context(pairs, r, ratios, cmax, device=DEV)
    assert _same_state(np.random.get_state(), want_state)
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert isinstance(a, np.ndarray) and a.dtype == b.dtype == np.int64 and a.shape == b.shape and np.array_equal(a, b)
    # the generator form, in the type the driver saves
    np.random.set_state(before)
    for a, b in zip(wide.iter_contexts(pairs, r, ratios, cmax, dtype=np.int16, device=DEV), want):
        assert a.dtype == np.int16 and a.flags["C_CONTIGUOUS"] and np.array_equal(a, b)
    assert _same_state(np.random.get_state(), want_state)
    # passing the cloud over: the same state, nothing returned
    np.random.set_state(before)
    assert wide.skip_contexts(len(pairs), r, ratios, cmax, DEV) is None
    assert _same_state(np.random.get_state(), want_state)


@pytest.mark.parametrize("r", [65, 128, 1024])
def test_context_regions_equal_the_rest_list(r):
    regions = np.arange(r)
    pairs = np.array([(0, 1), (0, r - 1), (r - 2, r - 1), (r // 2, r // 2 + 1), (r - 3, 2), (r - 1, r - 2)])
    rest = np.stack([regions[(regions != i) & (regions != j)] for i, j in pairs])
    rng = np.random.default_rng(r)
    for m in (0, 1, r - 2):
        heads = np.stack([np.stack([rng.permutation(r - 2)[:m] for _ in range(3)]) for _ in pairs]).astype(np.int32)
        if m == 1:
            heads[:, 0, 0], heads[:, 1, 0] = 0, r - 3
        dev = torch.from_numpy(heads).to(DEV)
        out = hip_ops.context_regions_wide(pairs, dev, r)
        assert out.data_ptr() == dev.data_ptr()          # in place
        want = np.take_along_axis(rest[:, None, :], heads.astype(np.int64), axis=2)
        assert np.array_equal(out.cpu().numpy(), want), (r, m)


def test_context_regions_wrapper_refuses_bad_pairs():
    heads = torch.zeros((1, 2, 3), dtype=torch.int32, device=DEV)
    for bad in ([[4, 4]], [[0, 128]], [[-1, 3]]):
        with pytest.raises(_lib.IqError):
            hip_ops.context_regions_wide(np.array(bad), heads, 128)
    with pytest.raises(_lib.IqError):
        hip_ops.context_regions_wide(np.array([[0, 1], [2, 3]]), heads, 128)          # two pairs, one row of heads
    with pytest.raises(_lib.IqError):
        hip_ops.context_regions_wide(np.array([[0, 1]]), torch.zeros((1, 1, 127), dtype=torch.int32, device=DEV), 128)
    with pytest.raises(_lib.IqError):
        hip_ops.context_regions_wide(np.array([[0, 1]]), heads, 1025)
    assert bool((heads == 0).all())


# ---- 2. the drivers ----

def _env():
    env = dict(os.environ, PYTHONPATH=REPO)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "IQ_FORCE_DIST", "IQ_REHEARSAL"):
        env.pop(k, None)
    return env


# four synthetic clouds: the interaction selection takes clouds 0 and 3, so the contexts of clouds 1 and 2 are passed over
COMMON = ["--model", "pointnet", "--dataset", "modelnet10", "--synthetic", "--num_clouds", "4", "--num_regions", "65"]
SAMPLERS = ("host", "device")


def _child(script, cwd, extra):
    gc.collect()
    torch.cuda.empty_cache()            # the child shares this GPU: hand back what the caching allocator holds
    run = subprocess.run([sys.executable, os.path.join(REPO, script)] + COMMON + extra, cwd=str(cwd), env=_env(), capture_output=True,
                         text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-3000:]


def _files(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def _assert_same_tree(a, b, expect):
    files = _files(a)
    assert files == _files(b) and files
    for name in expect:
        assert any(f.endswith(name) for f in files), (name, files[:20])
    for f in files:
        assert filecmp.cmp(os.path.join(a, f), os.path.join(b, f), shallow=False), f


@pytest.fixture(scope="module")
def stage1(tmp_path_factory):
    """final_wide_shapley.py, the smallest job it takes (65 regions, four permutations), once per sampler, each in one child."""
    dirs = {s: tmp_path_factory.mktemp("sampler_" + s) for s in SAMPLERS}
    for s in SAMPLERS:
        _child("final_wide_shapley.py", dirs[s], ["--num_samples_save", "4", "--sampler", s])
    return dirs


def test_final_wide_shapley_writes_the_same_files_with_either_sampler(stage1):
    _assert_same_tree(str(stage1["host"]), str(stage1["device"]), ["all_orders.npy", "region_sv_all.npy", "region_id.npy"])
    root = os.path.join(str(stage1["device"]), "checkpoints", "exp_MODEL_pointnet_DATA_modelnet10_POINTNUM_1024_REGIONNUM_65_shapley_test")
    orders = [np.load(os.path.join(root, "synthetic_%02d" % i, "all_orders.npy")) for i in range(4)]
    assert all(o.dtype == np.int64 and o.shape == (4, 65) and np.array_equal(np.sort(o, axis=1), np.tile(np.arange(65), (4, 1))) for o in orders)
    assert not np.array_equal(orders[0], orders[1])       # one stream running on from cloud to cloud


def test_final_wide_interaction_writes_the_same_files_with_either_sampler(stage1):
    for s in SAMPLERS:
        np.save(os.path.join(str(stage1[s]), "pose.npy"), np.array([0.4, -0.3, 0.2]))
        _child("final_wide_interaction.py", stage1[s], ["--num_pairs_random", "3", "--num_save_context_max", "4", "--mode", "rotate",
                                                        "--transform_params", "pose.npy", "--sampler", s])
    _assert_same_tree(str(stage1["host"]), str(stage1["device"]),
                      ["region_pair_list.npy", "ratio50_context_list.npy", "ratio90_context_list.npy", "ratio50_all_logits.pt",
                       "ratio50_pred_interaction.npy"])
    root = os.path.join(str(stage1["device"]), "checkpoints", "exp_MODEL_pointnet_DATA_modelnet10_POINTNUM_1024_REGIONNUM_65_shapley_test")
    for i in (0, 3):
        ctx = np.load(os.path.join(root, "synthetic_%02d" % i, "interaction_seed1", "ratio50_context_list.npy"))
        assert ctx.dtype == np.int16 and ctx.shape == (3, 4, 31)
    assert not os.path.exists(os.path.join(root, "synthetic_01", "interaction_seed1"))


def test_stage_one_passes_a_cloud_over_in_skip_mode(tmp_path, monkeypatch, capsys):
    """Cloud 2 alone: the permutations of clouds 0 and 1 are drawn and dropped (the device sampler's skip mode under --sampler
    device), so its all_orders.npy is the one of a run over all clouds."""
    from interpret_quality_amd import shapley_stage, wide_stage
    got = {}
    for s in SAMPLERS:
        work = tmp_path / s
        work.mkdir()
        monkeypatch.chdir(work)
        args = wide_stage.make_args(COMMON + ["--num_samples_save", "300", "--sampler", s])
        shapley_stage.finish_args(args)
        args.cloud_subset = {2}
        drawn = []
        monkeypatch.setattr(wide.__name__ + ".shapley", lambda *a, **k: drawn.append(a[4]) or ({}, np.zeros(1), None))
        wide_stage.run(args)
        got[s] = (drawn[0], np.random.get_state())
        assert not os.path.exists(os.path.join(args.exp_folder, "synthetic_00", "all_orders.npy"))
        assert np.array_equal(np.load(os.path.join(args.exp_folder, "synthetic_02", "all_orders.npy")), drawn[0])
    assert got["host"][0].dtype == got["device"][0].dtype == np.int64 and np.array_equal(got["host"][0], got["device"][0])
    assert _same_state(got["host"][1], got["device"][1])
    capsys.readouterr()
