"""Shared by tests/test_wide_pose_gpu.py and tests/test_wide_smoothness_gpu.py: the wide drivers run one after the other in ONE child
process (most of a launch is process start-up), on the synthetic cloud 0 of PointNet at 65 regions and 4 permutations."""
import json
import os
import subprocess
import sys

import torch

from conftest import REPO

REGIONS, SAMPLES = 65, 4
COMMON = ["--synthetic", "--num_clouds", "1", "--model", "pointnet", "--dataset", "modelnet10", "--num_regions", str(REGIONS)]
STAGE1 = COMMON + ["--num_samples_save", str(SAMPLES)]
POSE = STAGE1 + ["--num_samples", str(SAMPLES)]
EXP = os.path.join("checkpoints", "exp_MODEL_pointnet_DATA_modelnet10_POINTNUM_1024_REGIONNUM_%d_shapley_test" % REGIONS, "synthetic_00")
SCRIPTS = {"final_wide_shapley.py": "wide_stage", "final_wide_pose.py": "wide_pose_stage", "final_wide_smoothness.py": "wide_smoothness_stage",
           "final_wide_interaction.py": "wide_interaction_stage"}

_CHILD = """
import importlib, json, os, shutil, sys
for step in json.loads(sys.argv[1]):
    if "copytree" in step:
        shutil.copytree(*step["copytree"])
        continue
    os.chdir(step["cwd"])
    importlib.import_module("interpret_quality_amd." + step["module"]).main(step["argv"])
"""


def env():
    e = dict(os.environ, PYTHONPATH=REPO)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "IQ_FORCE_DIST", "IQ_REHEARSAL"):
        e.pop(k, None)
    return e


def step(cwd, script, argv):
    """One driver run: ``script`` is the root script's name; the child calls the main() that script calls."""
    return {"cwd": str(cwd), "module": SCRIPTS[script], "argv": list(argv)}


def run_child(steps, timeout=900):
    """The steps - driver runs (``step``) or {"copytree": [src, dst]} - in order in one fresh child process."""
    import gc
    gc.collect()
    if torch.cuda.is_available() and torch.cuda.is_initialized():
        torch.cuda.empty_cache()            # the child shares this GPU: hand back what the caching allocator holds
    r = subprocess.run([sys.executable, "-c", _CHILD, json.dumps(steps)], env=env(), capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    return r
