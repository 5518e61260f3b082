"""bench.py's `--dump-outputs` writer and the plain / --full defaults of its timing protocol, without a GPU."""
import importlib.util
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("iq_bench", os.path.join(REPO, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _written(d):
    return {f[:-4]: np.load(os.path.join(str(d), f)) for f in sorted(os.listdir(str(d)))}


def test_dump_outputs_writes_float32_or_float64_whole_below_the_cap(bench, tmp_path):
    arrays = {"phi_sum": np.linspace(-1, 1, 32), "logits": np.random.RandomState(1).rand(3300, 10).astype(np.float32),
              "orders": np.tile(np.arange(32, dtype=np.int32), (100, 1))}
    bench.dump_outputs(str(tmp_path), arrays)
    got = _written(tmp_path)
    assert set(got) == set(arrays)
    assert got["logits"].dtype == np.float32 and got["phi_sum"].dtype == np.float64 and got["orders"].dtype == np.float64
    for k in arrays:
        assert np.array_equal(got[k], arrays[k])


def test_dump_outputs_samples_the_same_rows_of_large_outputs_and_stays_under_64_mb(bench, tmp_path):
    logits = np.random.RandomState(2).rand(2_000_000, 10).astype(np.float32)      # 80 MB alone
    arrays = {"phi_sum": np.linspace(-1, 1, 32), "logits": logits, "orders": np.arange(64, dtype=np.int32).reshape(2, 32)}
    for tag in ("a", "b"):
        bench.dump_outputs(str(tmp_path / tag), arrays)
    a, b = _written(tmp_path / "a"), _written(tmp_path / "b")
    assert set(a) == set(b) == {"phi_sum", "logits", "logits_rows", "orders"}
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert sum(os.path.getsize(str(tmp_path / "a" / f)) for f in os.listdir(str(tmp_path / "a"))) <= 64 * 10 ** 6
    rows = a["logits_rows"].astype(np.int64)
    assert np.array_equal(a["logits_rows"], rows) and (np.diff(rows) > 0).all() and len(rows) > logits.shape[0] // 2
    assert np.array_equal(a["logits"], logits[rows])
    assert np.array_equal(a["phi_sum"], arrays["phi_sum"]) and np.array_equal(a["orders"], arrays["orders"])   # small ones whole


@pytest.mark.parametrize("argv,want", [([], (1, 0.0)), (["--full"], (5, 2.0)), (["--repeats", "3"], (3, 0.0)),
                                       (["--full", "--min-region-s", "0"], (5, 0.0))])
def test_a_plain_run_times_one_block_of_exactly_its_steps(bench, monkeypatch, argv, want):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "7"] + argv)
    args = bench.parse()
    assert args.steps == 7 and (args.repeats, args.min_region_s) == want and args.full == ("--full" in argv)
