"""GPU: a plain `bench.py` run (no --full) - exactly --steps timed steps, the headline line only - and `--dump-outputs`:
two runs with the same arguments write the same outputs, and those outputs satisfy the efficiency axiom."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R, S, STEPS = 32, 100, 3


def _env():
    env = dict(os.environ, PYTHONPATH=REPO)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "IQ_FORCE_DIST", "IQ_REHEARSAL", "IQ_BENCH_REHEARSAL"):
        env.pop(k, None)
    return env


@pytest.fixture(scope="module")
def plain_runs(tmp_path_factory):
    """Two plain launches with the same arguments, side by side (most of a launch is process start-up)."""
    if torch.cuda.is_available() and torch.cuda.is_initialized():
        import gc
        gc.collect()
        torch.cuda.empty_cache()   # the children share the GPU with this process
    root = tmp_path_factory.mktemp("bench_plain")
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", str(STEPS), "--warmup", "1", "--perms", str(S)]
    procs = [subprocess.Popen(cmd + ["--dump-outputs", str(root / tag)], cwd=str(root), env=_env(), stdout=subprocess.PIPE,
                              stderr=subprocess.PIPE, text=True) for tag in ("a", "b")]
    runs = []
    for tag, p in zip(("a", "b"), procs):
        out, err = p.communicate(timeout=600)
        assert p.returncode == 0, err[-3000:]
        lines = [ln for ln in out.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, out[-2000:]
        runs.append((json.loads(lines[0]), root / tag))
    return runs


def test_plain_bench_times_exactly_its_steps_and_prints_the_headline_only(plain_runs):
    for d, _ in plain_runs:
        assert d["unit"] == "coalitions/s" and d["higher_is_better"] is True and d["dtype"] == "f32" and d["scaling"] == "weak"
        assert "PointNet" in d["metric"] and d["n_gpus"] == 1 and d["steps"] == STEPS and d["warmup"] == 1
        t = d["timing"]
        assert t["blocks_s"] == t["regions_s"] and len(t["blocks_s"]) == 1           # one block of exactly --steps steps
        assert abs(d["ms_per_step"] * STEPS * 1e-3 - t["blocks_s"][0]) < 1e-9
        assert abs(d["value"] - S * (R + 1) * 1e3 / d["ms_per_step"]) < 1e-6 * d["value"]
        assert not {"roofline", "strong_scaling", "other_models", "gpu_eager_baseline", "cpu_baseline"} & set(d)


def test_dump_outputs_are_the_same_from_run_to_run(plain_runs):
    (_, a), (_, b) = plain_runs
    want = {"phi_sum": ((R,), np.float64), "sv_rows": ((S, R), np.float64), "logits": ((S * (R + 1), 10), np.float32),
            "reward": ((S * (R + 1),), np.float32), "orders": ((S, R), np.float64)}
    assert sorted(os.listdir(str(a))) == sorted(os.listdir(str(b))) == sorted(k + ".npy" for k in want)
    for k, (shape, dtype) in want.items():
        x, y = np.load(str(a / (k + ".npy"))), np.load(str(b / (k + ".npy")))
        assert x.shape == shape and x.dtype == dtype, (k, x.shape, x.dtype)
        np.testing.assert_allclose(x, y, rtol=1e-6, atol=1e-6 * np.abs(y).max(), err_msg=k)
    orders = np.load(str(a / "orders.npy"))
    assert (np.sort(orders, axis=1) == np.arange(R)).all()                            # every row a permutation
    # efficiency axiom on the dumped step: sum over regions of phi = v(all) - v(none) for every permutation
    phi_sum, sv_rows, v = (np.load(str(a / (k + ".npy"))) for k in ("phi_sum", "sv_rows", "reward"))
    v = v.astype(np.float64).reshape(S, R + 1)
    np.testing.assert_allclose(sv_rows.sum(axis=1), v[:, R] - v[:, 0], rtol=0, atol=1e-3)
    np.testing.assert_allclose(phi_sum, sv_rows.sum(axis=0), rtol=1e-12, atol=1e-9)
