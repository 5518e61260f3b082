"""GPU: --se through the three drivers that publish sampled estimates, each in child processes on --synthetic: the files the flag
adds, their shapes and symmetry, the z_rms keys, and that every other artefact keeps its bytes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLOUDS = ("synthetic_00", "synthetic_01")
COMMON = ["--model", "pointnet", "--dataset", "modelnet10", "--synthetic", "--num_clouds", "2"]


def _run(script, cwd, extra):
    cwd.mkdir(exist_ok=True)
    r = subprocess.run([sys.executable, os.path.join(REPO, script)] + COMMON + extra, cwd=str(cwd), env=dict(os.environ, PYTHONPATH=REPO),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]


def _folder(root, regions, cloud, stage):
    return root / "checkpoints" / ("exp_MODEL_pointnet_DATA_modelnet10_POINTNUM_1024_REGIONNUM_%d_shapley_test" % regions) / cloud / stage


def _differing(a, b, added):
    """The files of ``b`` (the run without --se) whose bytes differ in ``a``, which holds ``added`` beside them and nothing else."""
    names = sorted(os.listdir(b))
    assert sorted(os.listdir(a)) == sorted(names + list(added)), (sorted(os.listdir(a)), names)
    return [n for n in names if (a / n).read_bytes() != (b / n).read_bytes()]


def _is_a_bar(se, shape):
    assert se.shape == shape and se.dtype == np.float64 and np.all(np.isfinite(se)) and np.all(se >= 0)


def test_final_kernel_shapley_with_se(tmp_path):
    flags = ["--num_regions", "8", "--samples", "512", "--gram", "analytic", "--pairs", "--compare_exact"]
    _run("final_kernel_shapley.py", tmp_path / "with", flags + ["--se"])
    _run("final_kernel_shapley.py", tmp_path / "without", flags)
    for cloud in CLOUDS:
        a, b = (_folder(tmp_path / w, 8, cloud, "kernelshap") for w in ("with", "without"))
        assert _differing(a, b, ["region_shapley_se.npy", "region_interaction_se.npy"]) == ["sampling_error.json"]
        ja, jb = json.load(open(a / "sampling_error.json")), json.load(open(b / "sampling_error.json"))
        z_phi, z_pairs = ja.pop("z_rms"), ja["pairs"].pop("z_rms")
        assert ja == jb and "z_rms" not in jb and "z_rms" not in jb["pairs"]
        assert np.isfinite(z_phi) and z_phi > 0 and np.isfinite(z_pairs) and z_pairs > 0
        print("%s: z_rms %.3f (values), %.3f (pairs)" % (cloud, z_phi, z_pairs))
        _is_a_bar(np.load(a / "region_shapley_se.npy"), (8,))
        se = np.load(a / "region_interaction_se.npy")
        _is_a_bar(se, (8, 8))
        assert np.array_equal(se, se.T) and not np.diag(se).any() and np.all(se[np.triu_indices(8, 1)] > 0)


def test_final_wide_kernel_shapley_with_se(tmp_path):
    flags = ["--num_regions", "65", "--samples", "2000", "--draw", "counter", "--pairs"]
    _run("final_wide_kernel_shapley.py", tmp_path / "with", flags + ["--se"])
    _run("final_wide_kernel_shapley.py", tmp_path / "without", flags)
    for cloud in CLOUDS:
        a, b = (_folder(tmp_path / w, 65, cloud, "kernelshap") for w in ("with", "without"))
        assert _differing(a, b, ["region_shapley_se.npy", "region_interaction_se.npy"]) == ["draw.json"]
        ja, jb = json.load(open(a / "draw.json")), json.load(open(b / "draw.json"))
        assert ja.pop("se") is True and ja == jb
        _is_a_bar(np.load(a / "region_shapley_se.npy"), (65,))
        se = np.load(a / "region_interaction_se.npy")
        _is_a_bar(se, (65, 65))
        assert np.array_equal(se, se.T) and not np.diag(se).any() and np.all(se[np.triu_indices(65, 1)] > 0)


def test_final_class_shapley_with_se(tmp_path):
    flags = ["--num_regions", "8"]
    _run("final_shapley_value.py", tmp_path, flags + ["--num_samples_save", "100"])
    _run("final_class_shapley.py", tmp_path, flags + ["--num_samples", "100"])
    plain = {c: {n: (_folder(tmp_path, 8, c, "classwise") / n).read_bytes() for n in os.listdir(_folder(tmp_path, 8, c, "classwise"))} for c in CLOUDS}
    _run("final_class_shapley.py", tmp_path, flags + ["--num_samples", "100", "--se"])
    for i, cloud in enumerate(CLOUDS):
        folder = _folder(tmp_path, 8, cloud, "classwise")
        assert sorted(os.listdir(folder)) == sorted(list(plain[cloud]) + ["region_shapley_classes_se.npy"])
        assert [n for n in plain[cloud] if (folder / n).read_bytes() != plain[cloud][n]] == ["classes.json"]
        info = json.load(open(folder / "classes.json"))
        assert info.pop("se") is True and info == json.loads(plain[cloud]["classes.json"])
        phi, se = np.load(folder / "region_shapley_classes.npy"), np.load(folder / "region_shapley_classes_se.npy")
        _is_a_bar(se, phi.shape)
        rows = np.load(_folder(tmp_path, 8, cloud, "") / "region_sv_all.npy")     # stage 1's per-permutation rows, ground-truth label
        want = rows[:100].std(axis=0, ddof=1) / 10.0
        assert np.allclose(se[info["label"]], want, rtol=1e-9, atol=0.0)
