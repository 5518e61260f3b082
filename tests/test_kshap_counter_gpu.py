"""GPU: the counter-based draw of a wide game's rows (csrc/iq_kshap_draw.hip) against the NumPy restatement of its contract
(tests/kshap_counter_ref.py), bit for bit: rows and sizes over the edges of the word count, of the blocks of four regions and of
the four samples of a workgroup; forced sizes; the tie of two 32-bit keys; independence of the chunking; refusals; repeatability;
the estimator on such rows through PointNet; the driver's ``--draw counter``.  Nothing here is statistical."""
import argparse
import ctypes
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import kshap_counter_ref as ref
import probes
import wide_kernelshap_ref as wide_ref
from interpret_quality_amd import _lib, hip_ops, synth, wide_kernelshap

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

REGIONS = [2, 3, 5, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000, 1023, 1024]
COUNTS = [1, 3, 4, 5, 257]
FIRSTS = [0, 1, (1 << 32) - 2, (1 << 40) + 3]
SEEDS = [1, 0x9E3779B97F4A7C15]          # the second carries bits above 32: the key takes the low word
STREAMS = [0, 7]


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _draw(seed, stream, first, count, r, cdf=None, paired=True):
    keep, sizes = hip_ops.kshap_draw_counter(seed, stream, first, count, r, cdf, paired, DEV)
    assert keep.dtype == torch.int64 and sizes.dtype == torch.int32 and keep.device == DEV == sizes.device
    return _u64(keep), sizes.cpu().numpy()


def _popcount(rows):
    return np.unpackbits(np.ascontiguousarray(rows).view(np.uint8), axis=1).sum(axis=1)


def _forced(r, k):
    """A size table of k - 1 zeros followed by ones: every u gives size k."""
    cdf = np.ones(r - 1)
    cdf[:k - 1] = 0.0
    return cdf


# ---- rows and sizes, bit for bit ----

@pytest.mark.parametrize("r", REGIONS)
def test_rows_and_sizes_are_the_restatements(r):
    """Every count of COUNTS at this region count; paired or not, first, seed and stream picked per case by a seeded generator, so
    that over the 75 cases every value meets every region-count class and every count."""
    w = (r + 63) // 64
    for count in COUNTS:
        rng = np.random.default_rng(1000 * r + count)
        paired, first = bool(rng.integers(2)), FIRSTS[rng.integers(4)]
        seed, stream = SEEDS[rng.integers(2)], STREAMS[rng.integers(2)]
        tag = (r, count, paired, first, seed, stream)
        got, sizes = _draw(seed, stream, first, count, r, paired=paired)
        want, want_sizes = ref.rows(seed, stream, first, count, r, paired)
        assert got.shape == ((2 * count if paired else count), w) and sizes.shape == (count,), tag
        assert np.array_equal(sizes, want_sizes), tag
        assert np.array_equal(got, want), tag
        if r & 63:
            assert not np.any(got[:, -1] >> np.uint64(r & 63)), "a bit at or above R"
        assert np.array_equal(_popcount(got[0::2] if paired else got), sizes), tag


def test_every_first_seed_stream_and_pairing_at_the_widest_game():
    """R = 1024 and 65, 5 samples (two workgroups, the second ragged): the whole product of FIRSTS, SEEDS, STREAMS and pairing."""
    for r in (65, 1024):
        for first in FIRSTS:
            for seed in SEEDS:
                for stream in STREAMS:
                    for paired in (True, False):
                        got, sizes = _draw(seed, stream, first, 5, r, paired=paired)
                        want, want_sizes = ref.rows(seed, stream, first, 5, r, paired)
                        assert np.array_equal(got, want) and np.array_equal(sizes, want_sizes), (r, first, seed, stream, paired)


@pytest.mark.parametrize("r", [2, 65, 1024])
def test_forced_sizes(r):
    full = hip_ops.region_words(np.arange(r), r)
    for k in sorted({k for k in (1, 2, 64, 65, r - 1) if 1 <= k <= r - 1}):
        cdf = _forced(r, k)
        got, sizes = _draw(1, 0, 0, 9, r, cdf=cdf)
        want, _ = ref.rows(1, 0, 0, 9, r, cdf=cdf)
        assert np.array_equal(sizes, np.full(9, k)) and np.array_equal(got, want), (r, k)
        pop = _popcount(got)
        assert np.array_equal(pop[0::2], np.full(9, k)) and np.array_equal(pop[1::2], np.full(9, r - k)), (r, k)
        assert np.array_equal(got[0::2] ^ got[1::2], np.broadcast_to(full, (9, len(full))))
        # a table handed over as a device tensor is the same table
        again, _ = _draw(1, 0, 0, 9, r, cdf=torch.from_numpy(cdf).to(DEV))
        assert np.array_equal(again, got)


def test_equal_32_bit_keys_are_split_by_the_region_index():
    """R = 1024, seed 1, stream 0, sample 2158: two regions share a 32-bit key.  With the size forced to end between them the
    lower index is in and the higher is out; one size less and one more match the restatement as well."""
    r, m = 1024, 2158
    keys = ref.region_keys(1, 0, m, 1, r)[0]
    values, counts = np.unique(keys, return_counts=True)
    assert (counts == 2).sum() == 1 and counts.max() == 2
    low, high = np.flatnonzero(keys == values[counts == 2][0])
    order = np.argsort(ref.composite_keys(1, 0, m, 1, r)[0], kind="stable")
    p = int(np.flatnonzero(order == low)[0])
    assert order[p + 1] == high and 1 <= p and p + 2 <= r - 1

    def bit(rows, i):
        return int(rows[0, i >> 6] >> np.uint64(i & 63)) & 1

    for size in (p, p + 1, p + 2):
        cdf = _forced(r, size)
        got, sizes = _draw(1, 0, m, 1, r, cdf=cdf)
        want, _ = ref.rows(1, 0, m, 1, r, cdf=cdf)
        assert sizes[0] == size and np.array_equal(got, want), size
        assert (bit(got, low), bit(got, high)) == {p: (0, 0), p + 1: (1, 0), p + 2: (1, 1)}[size], size


@pytest.mark.parametrize("r", [65, 1024])
def test_rows_do_not_depend_on_the_chunking(r):
    whole, sizes = _draw(5, 3, 0, 1000, r)
    parts = [_draw(5, 3, lo, n, r) for lo, n in ((0, 1), (1, 257), (258, 742))]
    assert np.array_equal(np.concatenate([p[0] for p in parts]), whole)
    assert np.array_equal(np.concatenate([p[1] for p in parts]), sizes)
    single, _ = _draw(5, 3, 258, 742, r, paired=False)
    assert np.array_equal(single, whole[2 * 258::2])


def test_refusals():
    lib = _lib.load()
    cdf = torch.from_numpy(wide_kernelshap.size_cdf(128)).to(DEV)
    keep = torch.zeros((8, 2), dtype=torch.int64, device=DEV)
    sizes = torch.zeros((4,), dtype=torch.int32, device=DEV)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    c, k, s = (ctypes.c_void_p(t.data_ptr()) for t in (cdf, keep, sizes))
    for r in (1, 1025):
        assert lib.iq_kshap_draw_counter(1, 0, 0, 4, r, c, 1, k, s, st) == -1 and b"outside 2..1024" in lib.iq_last_error()
        with pytest.raises(_lib.IqError):
            hip_ops.kshap_draw_counter(1, 0, 0, 4, r, device=DEV)
    assert lib.iq_kshap_draw_counter(1, 0, -1, 4, 128, c, 1, k, s, st) == -1 and b"first" in lib.iq_last_error()
    assert lib.iq_kshap_draw_counter(1, 0, (1 << 62) - 3, 4, 128, c, 1, k, s, st) == -1
    assert lib.iq_kshap_draw_counter(1, 0, 0, 4, 128, c, 1, None, s, st) == -1 and b"null pointer" in lib.iq_last_error()
    assert lib.iq_kshap_draw_counter(1, 0, 0, 4, 128, None, 1, k, s, st) == -1
    assert lib.iq_kshap_draw_counter(1, 0, 0, 0, 128, None, 1, None, None, st) == 0
    torch.cuda.synchronize()
    assert not keep.any() and not sizes.any(), "a refused call wrote"
    with pytest.raises(_lib.IqError):
        hip_ops.kshap_draw_counter(1, 0, -1, 4, 128, device=DEV)
    with pytest.raises(_lib.IqError, match="cdf"):
        hip_ops.kshap_draw_counter(1, 0, 0, 4, 128, cdf=np.ones(128), device=DEV)
    empty_keep, empty_sizes = hip_ops.kshap_draw_counter(1, 0, 0, 0, 128, device=DEV)
    assert empty_keep.shape == (0, 2) and empty_sizes.shape == (0,)
    # a null sizes pointer is allowed: the rows are the same; and the call after a refusal works
    assert lib.iq_kshap_draw_counter(1, 0, 0, 4, 128, c, 1, k, None, st) == 0
    want, _ = ref.rows(1, 0, 0, 4, 128)
    assert np.array_equal(_u64(keep), want)


def test_draw_counter_repeats_and_leaves_numpys_generator_alone():
    np.random.seed(77)
    before = np.random.get_state()
    keep, sizes = wide_kernelshap.draw_counter(1000, 600, seed=4, stream=2, device=DEV)
    again, sizes2 = wide_kernelshap.draw_counter(1000, 600, seed=4, stream=2, device=DEV)
    after = np.random.get_state()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:]
    assert keep.shape == (600, 16) and isinstance(sizes, np.ndarray) and sizes.dtype == np.int32 and sizes.shape == (300,)
    assert _u64(keep).tobytes() == _u64(again).tobytes() and sizes.tobytes() == sizes2.tobytes()
    want, want_sizes = ref.rows(4, 2, 0, 300, 1000)
    assert np.array_equal(_u64(keep), want) and np.array_equal(sizes, want_sizes)
    # samples: paired rounds down to even; unpaired draws that many; first moves the window
    odd, _ = wide_kernelshap.draw_counter(1000, 7, seed=4, stream=2, device=DEV)
    assert odd.shape == (6, 16) and np.array_equal(_u64(odd), want[:6])
    tail, tail_sizes = wide_kernelshap.draw_counter(1000, 10, seed=4, stream=2, paired=False, device=DEV, first=290)
    assert np.array_equal(_u64(tail), want[2 * 290::2]) and np.array_equal(tail_sizes, want_sizes[290:])


# ---- through PointNet ----

@pytest.mark.parametrize("n,r,samples", [(256, 65, 600), (1024, 1024, 64)])
def test_counter_drawn_wide_game_through_pointnet(n, r, samples):
    """The bars of tests/test_wide_kernelshap_gpu.py's sampled game: sum(phi) = v_full - v_empty within 1e-12 max|v|, phi the
    restatement's closed form on the returned rows and rewards within 1e-9 max|v|."""
    pts, y = synth.make_cloud(0, n)
    data = torch.from_numpy(np.ascontiguousarray(pts))[None].to(DEV)
    fps = hip_ops.fps(data, r)[0].contiguous()
    rid = hip_ops.region_assign_wide(data[0].contiguous(), fps).cpu().numpy().astype(np.int64)
    args = argparse.Namespace(model="pointnet", softmax_type="modified", num_points=n, num_regions=r, verbose=False)
    lbl = torch.tensor([y], device=DEV)
    model, _ = probes.coalition_model("pointnet", DEV)
    np.random.seed(31)
    before = np.random.get_state()
    phi, v_full, v_empty, running = wide_kernelshap.shapley(model, data, lbl, rid, args, samples=samples, counts=[samples // 2, samples],
                                                            draw="counter", seed=6, stream=3)
    g = wide_kernelshap.game(model, data, lbl, rid, args, samples=samples, counts=[samples], draw="counter", seed=6, stream=3)
    after = np.random.get_state()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:]
    rows, vh = _u64(g["keep"]), g["v"].cpu().numpy()
    want_rows, _ = ref.rows(6, 3, 0, samples // 2, r)
    assert np.array_equal(rows, want_rows)
    assert np.array_equal(g["phi"], phi) and (g["v_full"], g["v_empty"]) == (v_full, v_empty)
    vmax = float(max(np.abs(vh).max(), abs(v_full), abs(v_empty)))
    want = wide_ref.estimate(rows, vh, v_empty, v_full, r)
    print("N=%d R=%d: max |phi - restatement| / max|v| = %.3g, |sum(phi) - delta| / max|v| = %.3g"
          % (n, r, np.abs(phi - want).max() / vmax, abs(math.fsum(phi) - (v_full - v_empty)) / vmax))
    assert phi.shape == (r,) and phi.dtype == np.float64
    assert np.abs(phi - want).max() <= 1e-9 * vmax
    assert abs(math.fsum(phi) - (v_full - v_empty)) <= 1e-12 * vmax
    assert sorted(running) == [samples // 2, samples] and np.array_equal(running[samples], phi)
    other = wide_kernelshap.game(model, data, lbl, rid, args, samples=samples, counts=[samples], draw="counter", seed=6, stream=4)
    assert not torch.equal(other["keep"], g["keep"])


# ---- driver ----

FLAGS = ["--model", "pointnet", "--dataset", "modelnet10", "--synthetic", "--num_clouds", "2", "--num_regions", "65", "--samples", "264",
         "--draw", "counter"]
ONE_CLOUD = ("import sys; from interpret_quality_amd import shapley_stage, wide_kernel_stage; "
             "args = wide_kernel_stage.make_args(sys.argv[1:]); shapley_stage.finish_args(args); args.cloud_subset = {1}; "
             "wide_kernel_stage.run(args)")


def _child(cwd, cmd):
    r = subprocess.run([sys.executable] + cmd + FLAGS, cwd=str(cwd), env=dict(os.environ, PYTHONPATH=REPO), capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


def test_driver_with_the_counter_draw_writes_a_cloud_alone_as_among_others(tmp_path):
    from interpret_quality_amd import wide_kernel_stage
    both, alone = tmp_path / "both", tmp_path / "alone"
    both.mkdir()
    alone.mkdir()
    _child(both, [os.path.join(REPO, "final_wide_kernel_shapley.py")])
    _child(alone, ["-c", ONE_CLOUD])
    folder = os.path.join("checkpoints", "exp_MODEL_pointnet_DATA_modelnet10_POINTNUM_1024_REGIONNUM_65_shapley_test")
    for name in wide_kernel_stage.FILES:
        a = (both / folder / "synthetic_01" / "kernelshap" / (name + ".npy")).read_bytes()
        b = (alone / folder / "synthetic_01" / "kernelshap" / (name + ".npy")).read_bytes()
        assert a == b, name
    assert not (alone / folder / "synthetic_00" / "kernelshap").exists()
    for cloud in (0, 1):
        root = both / folder / ("synthetic_%02d" % cloud) / "kernelshap"
        keep = np.load(root / "coalitions.npy")
        want, _ = ref.rows(1, cloud, 0, 132, 65)                       # --seed defaults to 1; the stream is the cloud's index
        assert keep.dtype == np.uint64 and np.array_equal(keep, want), cloud
        assert json.loads((root / "draw.json").read_text()) == {"draw": "counter", "seed": 1, "stream": cloud}
    assert json.loads((alone / folder / "synthetic_01" / "kernelshap" / "draw.json").read_text()) == {"draw": "counter", "seed": 1, "stream": 1}
