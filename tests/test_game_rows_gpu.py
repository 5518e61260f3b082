"""The rows of a regression game through final_common.rewards_with_ends on the GPU: ``kernelshap.rewards`` (6 regions) and
``wide_kernelshap.rewards`` (65 regions) of 20 drawn rows of a 128-point cloud, synthetic PointNet.  With the two end rows a call
scores 22: chunk 1 puts each end row into a launch of its own, chunk 5 (22 = 4 x 5 + 2) splits the end rows from the drawn rows
in a ragged last chunk, chunk 22 is one launch of exactly all rows, 1 << 16 the default.  Nothing may depend on the chunk; the
table of all classes is the single-label call per label, bit for bit; the end rows are classwise.ends's."""
import argparse

import numpy as np
import pytest
import torch

import probes
from interpret_quality_amd import classwise, hip_ops, kernelshap, synth, wide_kernelshap

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
CHUNKS = (1, 5, 22, 1 << 16)
_CACHE = {}


def _rows(r):
    """(estimator module, model, cloud, region ids, args, the 20 drawn rows) - and every result, computed once and shared."""
    if r not in _CACHE:
        ks = kernelshap if r <= kernelshap.MAX_REGIONS else wide_kernelshap
        model, _ = probes.coalition_model("pointnet", DEV)
        pts, _ = synth.make_cloud(0, 128)
        data = torch.from_numpy(np.ascontiguousarray(pts))[None].to(DEV)
        rid = hip_ops.region_assign_wide(data[0].contiguous(), hip_ops.fps(data, r)[0].contiguous()).cpu().numpy().astype(np.int64)
        args = argparse.Namespace(model="pointnet", softmax_type="modified", num_points=128, num_regions=r, verbose=False)
        state = np.random.get_state()
        np.random.seed(600 + r)
        keep, _ = ks.draw(r, 20, True, DEV)
        np.random.set_state(state)
        assert keep.shape[0] == 20
        single = {c: ks.rewards(model, data, torch.tensor([0], device=DEV), rid, args, keep, chunk=c) for c in CHUNKS}
        every = {c: ks.rewards(model, data, None, rid, args, keep, chunk=c, classes="all") for c in CHUNKS}
        _CACHE[r] = (ks, model, data, rid, args, keep, single, every)
    return _CACHE[r]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    """(v, v_full, v_empty) of two calls: the same shapes, types and bits."""
    if not (a[0].shape == b[0].shape and a[0].dtype == b[0].dtype == torch.float32 and torch.equal(_bits(a[0]), _bits(b[0]))):
        return False
    for x, y in zip(a[1:], b[1:]):
        x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
        if x.shape != y.shape or not np.array_equal(x.view(np.int64), y.view(np.int64)):
            return False
    return True


@pytest.mark.parametrize("r", [6, 65])
def test_rewards_do_not_depend_on_the_chunk(r):
    _, _, _, _, _, _, single, every = _rows(r)
    v, v_full, v_empty = single[1 << 16]
    assert v.shape == (20,) and isinstance(v_full, float) and isinstance(v_empty, float)
    table, t_full, t_empty = every[1 << 16]
    g = table.shape[0]
    assert g >= 2 and table.shape == (g, 20) and t_full.shape == t_empty.shape == (g,) and t_full.dtype == t_empty.dtype == np.float64
    for chunk in CHUNKS:
        assert _same(single[chunk], single[1 << 16]), chunk
        assert _same(every[chunk], every[1 << 16]), chunk


@pytest.mark.parametrize("r", [6, 65])
def test_row_g_of_all_classes_is_the_single_label_call(r):
    ks, model, data, rid, args, keep, single, every = _rows(r)
    g = every[1][0].shape[0]
    for label in range(g):
        for chunk in CHUNKS:
            want = single[chunk] if label == 0 else ks.rewards(model, data, torch.tensor([label], device=DEV), rid, args, keep, chunk=chunk)
            table, t_full, t_empty = every[chunk]
            assert _same((table[label], t_full[label], t_empty[label]), want), (label, chunk)
    sub = ks.rewards(model, data, None, rid, args, keep, chunk=5, classes=[g - 1, 0, g - 1])
    table, t_full, t_empty = every[5]
    assert _same(sub, (table[[g - 1, 0, g - 1]], t_full[[g - 1, 0, g - 1]], t_empty[[g - 1, 0, g - 1]]))


@pytest.mark.parametrize("r", [6, 65])
def test_end_rows_are_classwise_ends(r):
    _, model, data, rid, args, _, single, every = _rows(r)
    want_full, want_empty, _ = classwise.ends(model, data, rid, args)
    for chunk in CHUNKS:
        _, t_full, t_empty = every[chunk]
        assert np.array_equal(t_full.view(np.int64), want_full.view(np.int64)), chunk
        assert np.array_equal(t_empty.view(np.int64), want_empty.view(np.int64)), chunk
        _, v_full, v_empty = single[chunk]
        assert (v_full, v_empty) == (want_full[0], want_empty[0]), chunk
