"""GPU: one launch at the cap of every capped route (tests/launch_span.py: ``routes()``), every row bit for bit against the same
rows from launches of 64.

At ``max_clouds_per_call`` = 4096 coalitions the workspaces of PointNet++, PointConv and DGCNN / GCNN are 12 to 37 GiB, so inside
ONE production launch a per-coalition array crosses 2 GiB (``num_records`` of the raw buffer resources), 4 GiB (a 32-bit byte
offset) and 8 GiB (an ``int`` index of floats).  A narrow index does not fault there: the late coalitions get zeros or another
coalition's rows and plausible, wrong logits.  The suite's other tests compare launches below 1 GiB (PointConv), blocks of 660
against 3300 (PointNet++, narrow entry only) or "same set, same bits" (DGCNN, narrow entry only); the dense forwards, the wide and
compact entries, PointConv's cached tables and GCNN are held past the boundaries here only.  PointNet is out of scope: it has no
launch cap of this kind, 33 000 of its coalitions take 0.99 GiB and reach no boundary.

Per case: four seeded clouds, FPS regions (32; the wide and compact routes 128), 4096 seeded keep masks of every density and a
seeded ``cloud_of``; for ``forward_points`` the 4096 clouds those masks leave.  The big launch is asserted to be ONE launch in a
workspace of exactly the table's size (a silent split would make the comparison vacuous); the reference is the same call with
``max_clouds_per_call`` = 64.  ``rows_differ`` must return nothing, and the reference rows must be pairwise distinct bitwise except
where (cloud, kept set) coincide - otherwise a row that landed on another coalition's data could go unseen.  A twin is selected
for both launches.  ``coalition_logits`` of PointConv builds its per-cloud tables in the big launch; ``coalition_logits_cached``
finds them built by a launch of 64 on the same tensors and workspace.  The engine's workspace is dropped before and after every
case, so the peak is one family's workspace (PointConv: 36.2 GiB, what tests/test_pointconv_gpu.py already takes).

No case skips for lack of memory: it fails and says how much ``workspace.available_bytes`` found.

Measured on an MI355X (profiles/launch_span.txt): all 23 cases equal bit for bit - every route is clean today; the file takes 23 s,
a case 0.1 - 1.1 s of its own work (up to 4.4 s where it is the first in the process to launch its kernels).
"""
import argparse
import time

import numpy as np
import pytest
import torch

import launch_span as L
import probes
from interpret_quality_amd import hip_ops, synth, tuning, wide, workspace

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SMALL = 64      # the reference's launch size
# The ids of launch_span.routes(), written out: they carry the cap, the cloud size and the widest boundary crossed, so a changed
# cap or size formula makes this list stale and tests/test_launch_span_cpu.py says so.
CASES = [
    "pointnet2-forward_points-B4096-N128-8GiB",
    "pointnet2-forward_points-group_fp32-B4096-N128-8GiB",
    "pointnet2-coalition_logits-B4096-N128-8GiB",
    "pointnet2-coalition_logits-pn2_member_walk-B4096-N128-8GiB",
    "pointnet2-coalition_logits_wide-B4096-N128-8GiB",
    "pointnet2-compact-B4096-N128-8GiB",
    "pointconv-forward_points-B4096-N64-8GiB",
    "pointconv-forward_points-group_fp32-B4096-N64-8GiB",
    "pointconv-coalition_logits-B4096-N64-8GiB",
    "pointconv-coalition_logits-pc_two_kernel-B4096-N64-8GiB",
    "pointconv-coalition_logits_cached-B4096-N64-8GiB",
    "pointconv-coalition_logits_wide-B4096-N128-8GiB",
    "pointconv-compact-B4096-N128-8GiB",
    "dgcnn-forward_points-B4096-N1024-8GiB",
    "dgcnn-coalition_logits-B4096-N1024-8GiB",
    "dgcnn-coalition_logits-edge_gemm_l2-B4096-N1024-8GiB",
    "dgcnn-coalition_logits-edge_gemm_lds-B4096-N1024-8GiB",
    "dgcnn-coalition_logits_wide-B4096-N1024-8GiB",
    "dgcnn-compact-B4096-N1024-8GiB",
    "gcnn-forward_points-B4096-N1024-8GiB",
    "gcnn-coalition_logits-B4096-N1024-8GiB",
    "gcnn-coalition_logits_wide-B4096-N1024-8GiB",
    "gcnn-compact-B4096-N1024-8GiB",
]
_ROUTES, _INPUTS = {}, {}


def route_of(case):
    if not _ROUTES:
        _ROUTES.update({r.id: r for r in L.routes()})
    return _ROUTES[case]


def inputs(n, regions, b, nc):
    """Seeded inputs of a case, built once per (N, R, B, source clouds) and never written again: clouds (4,N,3), centers (4,3),
    rid (4,N) i32, keep (B,) or (B,W) i64 bit masks, cloud_of (B,) i32 or None (one cloud), key (B,) host (cloud, kept set) and -
    on demand, ``masked`` - the (B,N,3) clouds the masks leave."""
    if (n, regions, b, nc) in _INPUTS:
        return _INPUTS[(n, regions, b, nc)]
    rng = np.random.default_rng([n, regions, b, nc])
    count = max(nc, 1)
    clouds = torch.from_numpy(np.stack([synth.make_cloud(i, n)[0] for i in range(count)])).to(DEV).contiguous()
    assign = hip_ops.region_assign_wide if regions > 64 else hip_ops.region_assign
    rid = torch.stack([assign(clouds[c].contiguous(), hip_ops.fps(clouds[c:c + 1], regions)[0].contiguous()) for c in range(count)])
    # kept fractions from 5 % to 95 %: the compact paths' rows per coalition vary, and so does every prefix sum behind them
    member = rng.random((b, regions)) < rng.uniform(0.05, 0.95, size=(b, 1))
    # no empty coalition: the all-centre clouds of two centred source clouds are one cloud to within rounding, and their rows
    # could be bit-identical without anything being wrong
    for i in np.flatnonzero(~member.any(axis=1)):
        member[i, rng.integers(0, regions)] = True
    words = (regions + 63) // 64
    weights = np.left_shift(np.uint64(1), (np.arange(64 * words) & 63).astype(np.uint64))
    padded = np.zeros((b, 64 * words), dtype=bool)
    padded[:, :regions] = member
    rows = np.where(padded, weights, np.uint64(0)).reshape(b, words, 64).sum(axis=2, dtype=np.uint64)
    cloud_of = rng.integers(0, count, size=b).astype(np.int32)      # no period: a row copied from i - k meets another cloud
    d = {"clouds": clouds, "centers": clouds.mean(dim=1).contiguous(), "rid": rid.contiguous(),
         "keep": hip_ops.wide_masks_to_tensor(rows, DEV) if regions > 64 else hip_ops.masks_to_tensor(rows[:, 0], DEV),
         "cloud_of": torch.from_numpy(cloud_of).to(DEV) if count > 1 else None,
         "key": [(int(c),) + tuple(int(w) for w in row) for c, row in zip(cloud_of, rows)]}
    _INPUTS[(n, regions, b, nc)] = d
    return d


def masked_clouds(d, regions):
    """The (B,N,3) clouds of the keep masks: iq_mask_coalitions per source cloud, so the rows of the dense forward differ."""
    if "masked" not in d:
        b, n = d["keep"].shape[0], d["clouds"].shape[1]
        out = torch.empty((b, n, 3), dtype=torch.float32, device=DEV)
        for c in range(d["clouds"].shape[0]):
            sel = torch.nonzero(d["cloud_of"] == c).flatten()
            args = (d["clouds"][c].contiguous(), d["rid"][c].contiguous(), d["keep"][sel].contiguous(), d["centers"][c].contiguous())
            out[sel] = hip_ops.mask_coalitions_wide(*args, regions) if regions > 64 else hip_ops.mask_coalitions(*args)
        d["masked"] = out
    return d["masked"]


def launch(route, model, d, rows=None):
    """The route's call on all rows (or the first ``rows``) -> logits."""
    keep, cloud_of = d["keep"], d["cloud_of"]
    if rows is not None:
        keep, cloud_of = keep[:rows].contiguous(), None if cloud_of is None else cloud_of[:rows].contiguous()
    if route.route == "forward_points":
        return model.forward_points(masked_clouds(d, route.regions))
    if route.route in ("coalition_logits", "coalition_logits_cached"):
        return model.coalition_logits(d["clouds"], d["centers"], d["rid"], keep, cloud_of, num_regions=route.regions)
    if route.route == "coalition_logits_wide":
        return model.coalition_logits_wide(d["clouds"], d["centers"], d["rid"], keep, cloud_of, num_regions=route.regions)
    assert route.route == "compact" and cloud_of is None
    args = argparse.Namespace(model=route.family, num_regions=route.regions)
    return wide.coalition_logits(model, d["clouds"], d["rid"][0], keep, args, coalitions="compact")


def drop_workspace(eng):
    eng._ws = None
    eng.workspace_replaced()
    torch.cuda.empty_cache()


def undistinguished(ref, key):
    """Groups of positions whose reference rows carry the same bits although their (cloud, kept set) differ."""
    seen = {}
    for i, row in enumerate(ref.cpu().numpy().view(np.uint32)):
        seen.setdefault(row.tobytes(), []).append(i)
    return [g for g in seen.values() if len({key[i] for i in g}) > 1]


@pytest.mark.parametrize("case", CASES)
def test_every_row_of_a_launch_at_the_cap_equals_the_same_row_from_small_launches(case):
    route = route_of(case)
    model, _ = probes.coalition_model(route.family, DEV)
    assert type(model) is L.model_class(route.family) and model.max_clouds_per_call == route.cap
    eng = model.engine()
    d = inputs(route.n, route.regions, route.cap, route.nc or L.SOURCE_CLOUDS)
    if route.route == "forward_points":
        masked_clouds(d, route.regions)
    drop_workspace(eng)
    try:
        room = workspace.available_bytes(DEV)
        assert route.workspace_bytes <= room, "%s needs a workspace of %d bytes, workspace.available_bytes finds %d" % (
            case, route.workspace_bytes, room)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        with tuning.twin(route.twin):
            if route.route == "coalition_logits_cached":
                workspace.ensure(eng, route.workspace_bytes)                 # the tables live at the head of THIS workspace
                launch(route, model, d, SMALL)
                assert eng._tables_state(d["clouds"], d["centers"], route.nc, route.n) == 3, eng._tab.get("state")
            elif route.family == "pointconv" and route.nc:
                assert eng._tab == {}
            workspace.STATS["last_step"] = 0
            big = launch(route, model, d).clone()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            assert workspace.STATS["last_step"] == route.cap == big.shape[0], (workspace.STATS, big.shape)
            assert eng._ws.numel() == route.workspace_bytes, (eng._ws.numel(), route.workspace_bytes)
            if route.family == "pointconv" and route.nc:
                assert eng._tab.get("state") == 3, eng._tab.get("state")
                if route.route != "coalition_logits_cached":
                    eng._tab = {}                                            # the reference builds its own tables too
            model.max_clouds_per_call = SMALL
            try:
                ref = launch(route, model, d)
                assert workspace.STATS["last_step"] == SMALL, workspace.STATS
            finally:
                del model.max_clouds_per_call
        torch.cuda.synchronize()
        t2, peak = time.perf_counter(), torch.cuda.max_memory_allocated()
        # the allocation and the launch at the cap | the launches of 64 (profiles/launch_span.txt)
        print("launch_span %-62s nc %d R %3d workspace %11d bytes crosses %-14s %5.2f s + %5.2f s  peak %11d bytes" % (
            case, route.nc, route.regions, route.workspace_bytes, ",".join(route.crosses), t1 - t0, t2 - t1, peak))
        assert model.max_clouds_per_call == route.cap
        assert torch.isfinite(ref).all()
        bad = L.rows_differ(big, ref, route.bytes_per_coalition)
        assert bad == [], bad.message
        alike = undistinguished(ref, d["key"])
        assert not alike, "reference rows of different (cloud, kept set) carry the same bits: %s" % alike[:4]
    finally:
        drop_workspace(eng)
