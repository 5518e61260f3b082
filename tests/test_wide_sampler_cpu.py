"""CPU: what the device sampler for wide games has on the host - the ``rest`` formula of iq_context_regions_wide against the list
the reference builds, the --sampler flag of the wide drivers, the workspace query, and the device loop of gen_pair with a fake
``draw`` against the host loop (the order of ratios, which are enumerated, where the generator is handed back)."""
import re
import os

import numpy as np
import pytest

from interpret_quality_amd import _lib, gen_pair, hip_ops, wide, wide_interaction_stage, wide_pose_stage, wide_smoothness_stage, wide_stage
from interpret_quality_amd.interaction import DEFAULT_RATIOS

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _formula(k, i, j):
    """include/iq.h, iq_context_regions_wide: entry k of the ascending regions outside the pair."""
    lo, hi = min(i, j), max(i, j)
    return k + (k >= lo) + (k + 1 >= hi)


@pytest.mark.parametrize("r", [3, 4, 65, 128, 1024])
def test_the_rest_formula_is_the_list_the_reference_builds(r):
    regions = np.arange(r)
    pairs = {(0, 1), (0, r - 1), (r - 2, r - 1), (r // 2, r // 2 + 1), (1, r - 2), (r - 1, 0), (r // 3, 2 * r // 3)}
    for i, j in pairs:
        if i == j:
            continue
        rest = regions[(regions != i) & (regions != j)]          # final_gen_pair.py:25-27 (all_S), ascending
        k = np.arange(r - 2)
        assert np.array_equal(_formula(k, i, j), rest), (r, i, j)


def test_the_sampler_flag_parses_and_defaults_to_host():
    common = ["--model", "pointnet", "--dataset", "modelnet10", "--synthetic", "--num_regions", "128"]
    for make in (wide_stage.make_args, wide_interaction_stage.make_args):
        assert make(common).sampler == "host"
        assert make(common + ["--sampler", "device"]).sampler == "device"
        assert make(common + ["--sampler=host"]).sampler == "host"
        with pytest.raises(SystemExit):
            make(common + ["--sampler", "gpu"])
    assert wide_stage.SAMPLERS == ("host", "device")
    # scripts/exp_wide.sh hands one EXTRA to every wide stage: the stages that draw nothing take the flag too
    assert wide_pose_stage.make_args(common + ["--mode", "rotate", "--sampler", "device"]).sampler == "device"
    assert wide_smoothness_stage.make_args(common + ["--sampler", "device"]).sampler == "device"


def test_the_workspace_query():
    lib = _lib.load()
    for s, r in ((0, 128), (-3, 128), (10, 0), (10, 1), (10, 1025), (10, -1)):
        assert lib.iq_sample_wide_workspace_bytes(s, r) == 0, (s, r)
    assert lib.iq_sample_wide_workspace_bytes(2, 1024) == 0          # one batch of the one-workgroup kernel covers it
    for r in (2, 65, 128, 1022, 1024):
        sizes = [lib.iq_sample_wide_workspace_bytes(s, r) for s in (1, 2, 3, 7, 100, 300, 3000, 30000, 1000000)]
        assert sizes == sorted(sizes) and sizes[-1] > sizes[0] and all(b % 8 == 0 for b in sizes), (r, sizes)
    # 16 bytes per estimated word: 30 000 permutations of 1022 regions draw about 1411 words each
    assert 1405 < lib.iq_sample_wide_workspace_bytes(30000, 1022) / 16 / 30000 < 1425
    for r in (2, 32, 64):                                             # the narrow query's estimate
        assert lib.iq_sample_wide_workspace_bytes(1000, r) == lib.iq_sample_workspace_bytes(1000, r)


def test_the_call_size_search_of_the_wrapper():
    lib = _lib.load()
    for s, r, cap in ((30000, 1022, 128 << 20), (300, 1024, 1 << 20), (5, 1024, 1), (100, 65, 1 << 30)):
        n = hip_ops._wide_sample_call_size(lib, s, r, cap)
        assert 1 <= n <= s
        assert n == 1 or lib.iq_sample_wide_workspace_bytes(n, r) <= cap
        assert n == s or lib.iq_sample_wide_workspace_bytes(n + 1, r) > cap
    assert hip_ops._wide_sample_call_size(lib, 30000, 1022, hip_ops.SAMPLE_WIDE_WS_CAP) > 5000


def test_abi_113_declares_the_wide_sampler():
    header = open(os.path.join(REPO, "include", "iq.h")).read()
    version = int(re.search(r"#define IQ_ABI_VERSION (\d+)", header).group(1))
    lib = _lib.load()
    assert _lib.ABI_VERSION == lib.iq_version() == version >= 113
    for name in ("iq_sample_wide_workspace_bytes", "iq_sample_permutations_wide", "iq_context_regions_wide"):
        assert re.search(r"\b%s\s*\(" % name, header) and name in _lib.SIGNATURES and hasattr(lib, name)


@pytest.mark.parametrize("r,cmax", [(65, 100), (66, 5)])
def test_the_device_loop_with_a_host_draw_equals_the_host_loop(r, cmax, monkeypatch):
    """gen_pair.iter_contexts_device with a ``draw`` that draws on the host from the state it is handed: the arrays and NumPy's
    global state afterwards are the host loop's, the state goes out once and comes back once, and ``skip`` yields nothing but
    leaves the same state."""
    pairs = np.array([[0, 1], [r - 1, 3], [7, r - 2]])
    calls = {"up": 0, "down": 0}
    box = {}

    def to_device(dev, state=None):
        calls["up"] += 1
        box["state"] = np.random.get_state()
        return "the state"

    def to_host(state, set_global=True):
        calls["down"] += 1
        np.random.set_state(box["state"])

    def draw(state, prs, m, skip=False):
        assert state == "the state"
        np.random.set_state(box["state"])
        out = np.stack([np.stack([_formula(np.random.permutation(r - 2)[:m], i, j) for _ in range(cmax)]) for i, j in prs])
        box["state"] = np.random.get_state()
        np.random.seed(12345)                   # the global generator is not where the draws come from
        return None if skip else out

    monkeypatch.setattr(hip_ops, "mt_state_to_device", to_device)
    monkeypatch.setattr(hip_ops, "mt_state_to_host", to_host)
    np.random.seed(3)
    want = list(gen_pair.iter_contexts(pairs, r, DEFAULT_RATIOS, cmax))
    want_state = np.random.get_state()
    np.random.seed(3)
    got = list(gen_pair.iter_contexts_device(pairs, r, DEFAULT_RATIOS, cmax, "dev", draw))
    got_state = np.random.get_state()
    assert calls == {"up": 1, "down": 1}
    assert len(got) == len(want) == len(DEFAULT_RATIOS)
    for a, b in zip(got, want):
        assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)
    assert np.array_equal(got_state[1], want_state[1]) and got_state[2] == want_state[2]
    np.random.seed(3)
    skipped = list(gen_pair.iter_contexts_device(pairs, r, DEFAULT_RATIOS, cmax, "dev", lambda *a: draw(*a, skip=True), skip=True))
    assert skipped == [None] * len(DEFAULT_RATIOS)
    after = np.random.get_state()
    assert np.array_equal(after[1], want_state[1]) and after[2] == want_state[2]


def test_wide_iter_contexts_without_a_device_is_the_host_loop():
    pairs = np.array([[0, 64], [5, 3]])
    np.random.seed(9)
    want = list(gen_pair.iter_contexts(pairs, 65, DEFAULT_RATIOS, 4, np.int16))
    np.random.seed(9)
    got = list(wide.iter_contexts(pairs, 65, DEFAULT_RATIOS, 4, dtype=np.int16, device=None))
    assert all(a.dtype == np.int16 and np.array_equal(a, b) for a, b in zip(got, want)) and len(got) == len(want)
    np.random.seed(9)
    assert all(np.array_equal(a, b) for a, b in zip(wide.gen_context(pairs, 65, DEFAULT_RATIOS, 4, device=None), want))
