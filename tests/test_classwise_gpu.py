"""All-class games on the GPU: iq_reward_classes and iq_shapley_accum_games against the single-label entries per label / per game,
bit for bit; classwise.shapley / kernel_shapley / exact against today's single-label calls per label, bit for bit; the refusals;
the driver in one child process."""
import argparse
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import kernelshap_ref as ksref
import probes
from conftest import REPO
from interpret_quality_amd import _lib, classwise, exact, final_common, hip_ops, kernelshap, shapley_stage, synth, wide, wide_kernelshap
from interpret_quality_amd._lib import IqError

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SENTINEL = -12345.5


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def same_bits_np(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.int64 if a.dtype == np.float64 else np.int32),
                                                                        b.view(np.int64 if b.dtype == np.float64 else np.int32))


# ---- 1. reward_classes ------------------------------------------------------------------------------------------------------------

def _logits(b, c, seed):
    rng = np.random.RandomState(seed)
    z = (3.0 * rng.randn(b, c)).astype(np.float32)
    z[rng.rand(b, c) < 0.05] = -np.inf                      # rows holding -inf entries
    z[0] = -np.inf                                          # ... and one of nothing else
    if b > 3:
        z[1] = 1.25                                         # a row of equal values
        z[2] = np.where(np.arange(c) % 2 == 0, 80.0, -80.0)  # magnitudes of +-80
        z[3] = np.where(np.arange(c) % 3 == 0, -80.0, 79.5)
    return torch.from_numpy(z).to(DEV)


@pytest.mark.parametrize("modified", [True, False])
@pytest.mark.parametrize("c", [2, 3, 10, 40, 64])
def test_reward_classes_is_iq_reward_per_label(c, modified):
    for b in (1, 255, 256, 257, 1000):
        logits = _logits(b, c, 100 * c + b)
        single = torch.stack([hip_ops.reward(logits, label, modified) for label in range(c)])
        every = hip_ops.reward_classes(logits, None, modified)
        assert every.shape == (c, b) and same_bits(every, single), (b, c)
        sub = [c - 1, 0, c // 2, c - 1]                      # unsorted, with a repeat
        assert same_bits(hip_ops.reward_classes(logits, sub, modified), single[sub]), (b, c)
        # into a slice of a wider table: ldv = B + 7, the padding keeps its sentinel
        out = torch.full((len(sub), b + 7), SENTINEL, dtype=torch.float32, device=DEV)
        lib = _lib.load()
        lab = (ctypes.c_int32 * len(sub))(*sub)
        _lib.check(lib.iq_reward_classes(ctypes.c_void_p(logits.data_ptr()), lab, len(sub), int(modified), ctypes.c_void_p(out.data_ptr()),
                                         b + 7, b, c, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "iq_reward_classes")
        assert same_bits(out[:, :b], single[sub]) and bool((out[:, b:] == SENTINEL).all()), (b, c)
        # the wrapper's chunked form: two chunks at an offset fill the same table
        table = torch.full((c, b + 7), SENTINEL, dtype=torch.float32, device=DEV)
        cut = b // 2
        hip_ops.reward_classes(logits[:cut].contiguous(), None, modified, table, 3)
        hip_ops.reward_classes(logits[cut:].contiguous(), None, modified, table, 3 + cut)
        assert same_bits(table[:, 3:3 + b], single) and bool((table[:, :3] == SENTINEL).all()) and bool((table[:, 3 + b:] == SENTINEL).all())


@pytest.mark.parametrize("softmax_type", ["modified", "normal"])
def test_reward_classes_against_the_oracle(softmax_type):
    from oracle import ref_cpu
    z = torch.from_numpy((3.0 * np.random.RandomState(5).randn(300, 10)).astype(np.float32))
    got = hip_ops.reward_classes(z.to(DEV), None, softmax_type == "modified").cpu().numpy()
    for label in range(10):
        want = ref_cpu.get_reward(z, torch.tensor([label]), softmax_type).numpy()
        np.testing.assert_allclose(got[label], want, rtol=2e-6, atol=2e-6)       # tests/test_hip_parity.py::test_reward's bar


# ---- 2. shapley_accum_games -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("r", [1, 2, 63, 64, 65, 127, 128, 1000, 1024])
def test_shapley_accum_games_is_the_single_game_entry_per_game(r):
    rng = np.random.RandomState(1000 + r)
    gmax = 40
    for s in (1, 63, 64, 65, 129):
        per, ldv = s * (r + 1), s * (r + 1) + 5
        v = (2.0 * rng.randn(gmax, ldv)).astype(np.float32)
        if s > 2:
            v[:, :r + 1] = 1.5                                   # a permutation of equal rewards: differences of +0.0
            v[:, r + 1:2 * (r + 1)] = np.where(np.arange(r + 1) % 2 == 0, 0.0, -0.0).astype(np.float32)     # and of -0.0
        v = torch.from_numpy(v).to(DEV)
        orders = np.stack([rng.permutation(r) for _ in range(s)])
        orders_dev = hip_ops.as_i32(orders, DEV)
        counts = sorted({min(c, s) for c in (1, 64, 65, s)})
        want_phi, want_snaps = [], []
        for g in range(gmax):
            phi, _, snaps = hip_ops.shapley_accum_wide(v[g, :per], orders_dev, counts)
            if r <= 64:
                phi_n, _, snaps_n = hip_ops.shapley_accum(v[g, :per], orders_dev, counts)
                assert same_bits(phi_n, phi) and same_bits(snaps_n, snaps)
            want_phi.append(phi)
            want_snaps.append(snaps)
        want_phi, want_snaps = torch.stack(want_phi), torch.stack(want_snaps)
        assert bool((want_phi != 0).all())
        for g in (1, 3, gmax):
            phi, snaps = hip_ops.shapley_accum_games(v[:g], orders, counts)
            assert phi.shape == (g, r) and snaps.shape == (g, len(counts), r)
            assert same_bits(phi, want_phi[:g]) and same_bits(snaps, want_snaps[:g]), (r, s, g)
            again, snaps2 = hip_ops.shapley_accum_games(v[:g], orders_dev, counts)
            assert same_bits(again, phi) and same_bits(snaps2, snaps)
        assert hip_ops.shapley_games_scratch_bytes(r, s, 1) == hip_ops.shapley_games_scratch_bytes(r, s, gmax) > 0
        total, none = hip_ops.shapley_accum_games(v[:3], orders)
        assert none is None and same_bits(total, want_phi[:3])


def test_a_region_a_row_does_not_name_contributes_zero():
    r, s = 70, 3
    rng = np.random.RandomState(3)
    v = torch.from_numpy(rng.randn(2, s * (r + 1)).astype(np.float32)).to(DEV)
    orders = np.stack([rng.permutation(r) for _ in range(s)])
    orders[1, 5] = orders[1, 6]                              # row 1 names one region twice and another not at all
    lost = (set(range(r)) - set(orders[1].tolist())).pop()
    phi, _ = hip_ops.shapley_accum_games(v, orders)
    want = np.zeros((2, r))
    vh = v.cpu().numpy()
    for g in range(2):
        for o in range(s):
            row = vh[g, o * (r + 1):(o + 1) * (r + 1)]
            dv = (row[1:] - row[:-1]).astype(np.float64)
            for j in range(r):
                if not (o == 1 and j in (5, 6)):
                    want[g, orders[o, j]] += dv[j]
    keep = np.array([k for k in range(r) if k != orders[1, 5]])       # the twice-named region takes either difference
    assert same_bits_np(phi.cpu().numpy()[:, keep], want[:, keep])
    assert lost in keep


# ---- 3. classwise.shapley ----------------------------------------------------------------------------------------------------------

def _args(family, n, r):
    return argparse.Namespace(model=family, softmax_type="modified", num_points=n, num_regions=r, verbose=False)


_GAMES = {}


def _game(family, n, r):
    """Synthetic cloud 0 at its first n points, r regions from the device's own FPS."""
    if (family, n, r) not in _GAMES:
        pts, y = synth.make_cloud(0, n)
        data = torch.from_numpy(np.ascontiguousarray(pts))[None].to(DEV)
        fps = hip_ops.fps(data, r)[0].contiguous()
        rid = hip_ops.region_assign_wide(data[0].contiguous(), fps).cpu().numpy().astype(np.int64)
        _GAMES[(family, n, r)] = (data, y, rid, _args(family, n, r))
    return _GAMES[(family, n, r)]


def _lbl(c):
    return torch.tensor([c], device=DEV)


def test_classwise_shapley_narrow_is_stage_1_per_label():
    data, _, rid, args = _game("pointnet", 128, 8)
    model, _ = probes.coalition_model("pointnet", DEV)
    orders = np.stack([np.random.RandomState(11).permutation(8) for _ in range(4)])
    snaps, total = classwise.shapley(model, data, rid, orders, args, snap_counts=[1, 4, 100])
    c = total.shape[0]
    assert c >= 2 and total.shape == (c, 8) and total.dtype == np.float64 and sorted(snaps) == [1, 4]
    for label in range(c):
        _, rows, want = shapley_stage.shapley_all_orders(model, data, _lbl(label), rid, orders, args)
        assert same_bits_np(total[label], want), label
        assert same_bits_np(snaps[4][label], want) and same_bits_np(snaps[1][label], rows[0])
    sub_snaps, sub = classwise.shapley(model, data, rid, orders, args, classes=[c - 1, 0, c - 1])
    assert sub_snaps == {} and same_bits_np(sub, total[[c - 1, 0, c - 1]])
    with torch.no_grad():
        logits = final_common.shapley_logits(model, data, None, rid, orders, args)
    f_snaps, f_total = classwise.from_logits(logits, orders, args, snap_counts=[1, 4])
    assert same_bits_np(f_total, total) and all(same_bits_np(f_snaps[k], snaps[k]) for k in (1, 4))
    with pytest.raises(IqError):
        classwise.shapley(model, data, rid, orders, args, route="keep")


@pytest.mark.parametrize("r", [65, 128])
def test_classwise_shapley_wide_is_wide_shapley_per_label_on_both_routes(r):
    data, _, rid, args = _game("pointnet", 128, r)
    model, _ = probes.coalition_model("pointnet", DEV)
    orders = np.stack([np.random.RandomState(12 + r).permutation(r) for _ in range(4)])
    totals = {}
    for route in wide.ROUTES:
        snaps, total = classwise.shapley(model, data, rid, orders, args, snap_counts=[1, 4], route=route)
        for label in range(total.shape[0]):
            want_snaps, _, want = wide.shapley(model, data, _lbl(label), rid, orders, args, snap_counts=[1, 4], route=route)
            assert same_bits_np(total[label], want), (route, label)
            assert all(same_bits_np(snaps[k][label], want_snaps[k]) for k in (1, 4))
        totals[route] = total
    assert same_bits_np(totals["prefix"], totals["keep"])
    with torch.no_grad():
        logits = wide.prefix_logits(model, data, rid, orders, args)
    assert same_bits_np(classwise.from_logits(logits, orders, args)[1], totals["prefix"])


def test_classwise_shapley_of_another_family_through_the_dense_route():
    data, _, rid, args = _game("pointnet2", 128, 65)
    model, _ = probes.coalition_model("pointnet2", DEV)
    orders = np.stack([np.random.RandomState(13).permutation(65) for _ in range(2)])
    _, total = classwise.shapley(model, data, rid, orders, args, coalitions="dense")
    for label in range(total.shape[0]):
        _, _, want = wide.shapley(model, data, _lbl(label), rid, orders, args, coalitions="dense")
        assert same_bits_np(total[label], want), label


# ---- 4. classwise.kernel_shapley ---------------------------------------------------------------------------------------------------

def _identity_bound(n, vmax):
    """tests/test_kernelshap_gpu.py's bar on the enumeration identity for one label."""
    return 2.0 ** -23 * vmax + n * ksref.cond_analytic(n) * 2.0 ** -52 * vmax


def test_kernel_shapley_narrow_is_kernelshap_per_label_and_enumerated_is_exact():
    data, _, rid, args = _game("pointnet", 128, 6)
    model, _ = probes.coalition_model("pointnet", DEV)
    np.random.seed(41)
    phi, v_full, v_empty = classwise.kernel_shapley(model, data, rid, args, samples=64)
    c = phi.shape[0]
    assert phi.shape == (c, 6) and phi.dtype == np.float64 and v_full.shape == v_empty.shape == (c,)
    for label in range(c):
        np.random.seed(41)
        want, f, e, _ = kernelshap.shapley(model, data, _lbl(label), rid, args, samples=64)
        assert same_bits_np(phi[label], want) and (v_full[label], v_empty[label]) == (f, e), label
    every, _, _ = classwise.kernel_shapley(model, data, rid, args, samples="all")
    want, tables = classwise.exact(model, data, rid, args)
    for label in range(c):
        vmax = float(tables[label].abs().max())
        assert np.abs(every[label] - want[label]).max() <= _identity_bound(6, vmax), label


def test_kernel_shapley_wide_is_wide_kernelshap_per_label():
    data, _, rid, args = _game("pointnet", 128, 65)
    model, _ = probes.coalition_model("pointnet", DEV)
    phi, v_full, v_empty = classwise.kernel_shapley(model, data, rid, args, samples=64, draw="counter", seed=5, stream=2)
    assert phi.shape[1] == 65
    for label in range(phi.shape[0]):
        want, f, e, _ = wide_kernelshap.shapley(model, data, _lbl(label), rid, args, samples=64, draw="counter", seed=5, stream=2)
        assert same_bits_np(phi[label], want) and (v_full[label], v_empty[label]) == (f, e), label


# ---- 5. classwise.exact ------------------------------------------------------------------------------------------------------------

def test_exact_is_exact_shapley_per_label_and_guards_its_tables():
    data, _, rid, args = _game("pointnet", 128, 6)
    model, _ = probes.coalition_model("pointnet", DEV)
    phi, tables = classwise.exact(model, data, rid, args)
    c = phi.shape[0]
    assert phi.shape == (c, 6) and tables.shape == (c, 64) and tables.dtype == torch.float32
    for label in range(c):
        v = exact.value_table(model, data, _lbl(label), rid, args)
        want, _, _ = exact.shapley(model, data, _lbl(label), rid, args, v=v)
        assert same_bits(tables[label], v) and same_bits_np(phi[label], want), label
    sub, _ = classwise.exact(model, data, rid, args, classes=[3, 3, 1], players=[5, 0, 2], base=2)
    want, _, _ = exact.shapley(model, data, _lbl(3), rid, args, players=[5, 0, 2], base=2)
    assert same_bits_np(sub[0], want) and same_bits_np(sub[1], want)
    # c * 2^24 floats > 2^28 for every c > 16; the synthetic model has fewer classes, so name 17 labels: refused before the cloud
    # (None here) is ever looked at
    big = _args("pointnet", 128, 24)
    with pytest.raises(IqError, match="2\\^28"):
        classwise.exact(model, None, None, big, classes=[0] * 17)
    assert classwise.num_games(model, None) == c


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------

def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def test_refusals_launch_nothing():
    lib = _lib.load()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    b = 16
    logits = torch.zeros((b, 65), dtype=torch.float32, device=DEV)
    v = torch.full((65, b + 1), SENTINEL, dtype=torch.float32, device=DEV)
    lab = (ctypes.c_int32 * 3)(0, 10, 1)
    cases = {"C = 65": (None, 65, b, 65), "label == C": (lab, 3, b, 10), "labels NULL, G != C": (None, 3, b, 10),
             "ldv < B": (None, 10, b - 1, 10), "G = 0": (lab, 0, b, 10), "G = 65": (lab, 65, b, 10), "C = 1": (None, 1, b, 1)}
    for what, (labels, g, ldv, c) in cases.items():
        rc = lib.iq_reward_classes(_ptr(logits), labels, g, 1, _ptr(v), ldv, b, c, stream)
        assert rc != 0 and lib.iq_last_error(), what
        with pytest.raises(IqError):
            _lib.check(rc, what)
    torch.cuda.synchronize()
    assert bool((v == SENTINEL).all())
    assert lib.iq_reward_classes(_ptr(logits), None, 10, 1, _ptr(v), 0, 0, 10, stream) == 0          # B == 0 is IQ_OK
    with pytest.raises(IqError):
        hip_ops.reward_classes(logits[:, :10].contiguous(), [0, 10])
    with pytest.raises(IqError):
        hip_ops.reward_classes(logits[:, :10].contiguous(), None, True, v[:10, :b - 1].contiguous())

    r, s = 1025, 2
    vv = torch.zeros((1, s * (r + 1)), dtype=torch.float32, device=DEV)
    orders = torch.zeros((s, r), dtype=torch.int32, device=DEV)
    phi = torch.full((1, r), SENTINEL, dtype=torch.float64, device=DEV)
    scratch = torch.zeros((1 << 16,), dtype=torch.uint8, device=DEV)
    for what, (rr, g, ldv, nbytes) in {"R = 1025": (1025, 1, s * 1026, 1 << 16), "G = 0": (64, 0, s * 65, 1 << 16),
                                       "ldv < S*(R+1)": (64, 1, s * 65 - 1, 1 << 16), "short scratch": (64, 1, s * 65, 8)}.items():
        rc = lib.iq_shapley_accum_games(_ptr(vv), ldv, _ptr(orders), _ptr(phi), None, 0, None, rr, s, g, _ptr(scratch), nbytes, stream)
        assert rc != 0, what
    torch.cuda.synchronize()
    assert bool((phi == SENTINEL).all())
    with pytest.raises(IqError):
        hip_ops.shapley_accum_games(vv, np.zeros((s, r), dtype=np.int64))
    with pytest.raises(IqError):                              # an order entry outside [0, R), caught on the host
        hip_ops.shapley_accum_games(vv, np.full((2, 8), 8, dtype=np.int64))


# ---- 7. the driver -----------------------------------------------------------------------------------------------------------------

_CHILD = """
import final_shapley_value, final_class_shapley
common = ["--model", "pointnet", "--dataset", "modelnet10", "--synthetic", "--num_clouds", "2", "--num_regions", "8"]
final_shapley_value.main(common + ["--num_samples_save", "100"])
final_class_shapley.main(common + ["--num_samples", "100"])
"""


def test_driver_in_one_child_process(tmp_path):
    env = dict(os.environ, PYTHONPATH=REPO)
    run = subprocess.run([sys.executable, "-c", _CHILD], cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-3000:]
    base = tmp_path / "checkpoints" / "exp_MODEL_pointnet_DATA_modelnet10_POINTNUM_1024_REGIONNUM_8_shapley_test"
    model, _ = probes.coalition_model("pointnet", DEV)
    args = _args("pointnet", 1024, 8)
    for i, cloud in enumerate(("synthetic_00", "synthetic_01")):
        root = base / cloud
        phi = np.load(root / "classwise" / "region_shapley_classes.npy")
        eff = np.load(root / "classwise" / "efficiency.npy")
        info = json.load(open(root / "classwise" / "classes.json"))
        c = len(info["classes"])
        assert c == classwise.num_games(model, None) and info["classes"] == list(range(c))
        assert phi.shape == (c, 8) and phi.dtype == np.float64 and eff.shape == (c,)
        assert info["estimator"] == "permutation" and info["parameters"]["num_samples"] == 100
        pts, y = synth.make_cloud(i)
        assert info["label"] == int(y) and 0 <= info["predicted"] < c
        stage1 = np.load(root / "region_shapley" / ("%d_100.npy" % i))
        assert same_bits_np(phi[info["label"]], stage1)
        v_full, v_empty = np.array(info["v_full"]), np.array(info["v_empty"])
        assert np.array_equal(eff, phi.sum(axis=1) - (v_full - v_empty))
        # the bound of tests/test_classwise_cpu.py, on the rewards of this cloud's own game: phi is the total over S, so is the bar
        data = torch.from_numpy(pts)[None].to(DEV)
        orders, rid = np.load(root / "all_orders.npy"), np.load(root / "region_id.npy")
        with torch.no_grad():
            v = classwise.rewards(final_common.shapley_logits(model, data, None, rid, orders, args), None, args)
        bound = 8 * 2.0 ** -23 * v.abs().max(dim=1).values.cpu().numpy().astype(np.float64)
        print("cloud %d: max |efficiency| / bound = %.3g" % (i, (np.abs(eff) / bound).max()))
        assert (np.abs(eff) <= bound).all(), (eff, bound)
