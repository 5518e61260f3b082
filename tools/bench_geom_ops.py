#!/usr/bin/env python3
"""Time the standalone geometric ops (include/iq.h: iq_group_points, iq_edgeconv_gather, iq_knn_point, iq_density) against
the eager-PyTorch formulation of the same reference function on the same GPU, with torch.cuda events.

    python tools/bench_geom_ops.py [--reps 50] [--out profiles/geom_ops.json]

Shapes: PointNet++ sa1 / sa2 grouping at B = 33 (the largest scale of each: K = 128), get_graph_feature at C = 64 and 128
(B = 33, N = 1024, k = 20, idx given), PointConv's knn_point at 512 queries x 32 neighbours (B = 33, N = 1024) and
compute_density at N = 1024 (B = 33).  For the gathers, the effective rate counts the bytes a single pass must move: the
output written, the indices read and the source tensors read once.  The gathers are timed twice: as their launch
(hip_us), and through the Python wrapper with torch.long indices as models.* calls it (wrapper_us), which adds the index
validation - the int32 cast and iq_check_index_range, one stream synchronisation per call."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from interpret_quality_amd import hip_ops  # noqa: E402

B = 33


def eager_index_points(points, idx):     # models/pointnet2.py:27-43
    b = points.shape[0]
    view_shape = [b] + [1] * (idx.dim() - 1)
    repeat_shape = [1] + list(idx.shape[1:])
    batch = torch.arange(b, dtype=torch.long, device=points.device).view(view_shape).repeat(repeat_shape)
    return points[batch, idx, :]


def eager_square_distance(src, dst):     # models/pointconv.py:13-32
    b, n, _ = src.shape
    m = dst.shape[1]
    dist = -2 * torch.matmul(src, dst.permute(0, 2, 1))
    dist += torch.sum(src ** 2, -1).view(b, n, 1)
    dist += torch.sum(dst ** 2, -1).view(b, 1, m)
    return dist


def eager_graph_feature(x, k, idx):      # models/dgcnn.py:21-47 with idx given
    b, c, n = x.shape
    idx = (idx + torch.arange(0, b, device=x.device).view(-1, 1, 1) * n).view(-1)
    xt = x.transpose(2, 1).contiguous()
    feature = xt.view(b * n, -1)[idx, :].view(b, n, k, c)
    xt = xt.view(b, n, 1, c).repeat(1, 1, k, 1)
    return torch.cat((feature - xt, xt), dim=3).permute(0, 3, 1, 2)


def time_ms(fn, reps):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        e.record()
        e.synchronize()
        times.append(a.elapsed_time(e))
    times.sort()
    return times[len(times) // 2]


def nbytes(*ts):
    return sum(t.numel() * t.element_size() for t in ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    d = torch.device("cuda:0")
    g = torch.Generator(device=d).manual_seed(0)
    rows = []

    def record(name, shape, hip, eager, moved=None, wrapper=None):
        th, te = time_ms(hip, args.reps), time_ms(eager, args.reps)
        row = {"op": name, "shape": shape, "hip_us": round(th * 1e3, 2), "eager_us": round(te * 1e3, 2),
               "speedup": round(te / th, 2)}
        if wrapper is not None:
            tw = time_ms(wrapper, args.reps)
            row["wrapper_us"] = round(tw * 1e3, 2)
            row["wrapper_speedup"] = round(te / tw, 2)
        if moved is not None:
            row["moved_MB"] = round(moved / 1e6, 2)
            row["hip_GBps"] = round(moved / (th * 1e-3) / 1e9, 1)
        rows.append(row)
        print(json.dumps(row), flush=True)

    # PointNet++ sa1 (largest scale): relative xyz of 128 ball members around 512 centroids
    xyz = torch.rand((B, 1024, 3), device=d, generator=g)
    nx = xyz[:, :512].contiguous()
    idx = torch.randint(0, 1024, (B, 512, 128), device=d, generator=g, dtype=torch.int32)
    idx64 = idx.long()
    out = hip_ops.group_points(xyz, None, nx, idx)
    assert torch.equal(out, eager_index_points(xyz, idx64) - nx.view(B, 512, 1, 3))
    lib_group = lambda: hip_ops._lib.check(hip_ops._lib.load().iq_group_points(  # noqa: E731  (the launch alone: no validation sync)
        hip_ops._p(xyz), hip_ops._p(None), hip_ops._p(nx), hip_ops._p(idx), hip_ops._p(out), 1, B, 1024, 512, 128, 0,
        hip_ops._stream()), "iq_group_points")
    record("group sa1 (xyz - c)", [B, 512, 128, 3], lib_group, lambda: eager_index_points(xyz, idx64) - nx.view(B, 512, 1, 3),
           nbytes(out, idx, xyz, nx), lambda: hip_ops.group_points(xyz, None, nx, idx64))

    # PointNet++ sa2 (largest scale): [features (320), xyz - c] of 128 members around 128 centroids, features first
    xyz2 = torch.rand((B, 512, 3), device=d, generator=g)
    pts2 = torch.randn((B, 512, 320), device=d, generator=g)
    nx2 = xyz2[:, :128].contiguous()
    idx2 = torch.randint(0, 512, (B, 128, 128), device=d, generator=g, dtype=torch.int32)
    idx2_64 = idx2.long()
    out2 = hip_ops.group_points(xyz2, pts2, nx2, idx2, xyz_first=False)

    def eager_sa2():
        gx = eager_index_points(xyz2, idx2_64)
        gx -= nx2.view(B, 128, 1, 3)
        return torch.cat([eager_index_points(pts2, idx2_64), gx], dim=-1)
    assert torch.equal(out2, eager_sa2())
    lib_group2 = lambda: hip_ops._lib.check(hip_ops._lib.load().iq_group_points(  # noqa: E731
        hip_ops._p(xyz2), hip_ops._p(pts2), hip_ops._p(nx2), hip_ops._p(idx2), hip_ops._p(out2), 0, B, 512, 128, 128, 320,
        hip_ops._stream()), "iq_group_points")
    record("group sa2 ([f, xyz - c], D = 320)", [B, 128, 128, 323], lib_group2, eager_sa2, nbytes(out2, idx2, xyz2, pts2, nx2),
           lambda: hip_ops.group_points(xyz2, pts2, nx2, idx2_64, xyz_first=False))

    # DGCNN edge features, idx given
    for c in (64, 128):
        x = torch.randn((B, c, 1024), device=d, generator=g)
        ei = torch.randint(0, 1024, (B, 1024, 20), device=d, generator=g, dtype=torch.int32)
        ei64 = ei.long()
        eo = hip_ops.edgeconv_gather(x, ei)
        assert torch.equal(eo, eager_graph_feature(x, 20, ei64))
        lib_edge = lambda: hip_ops._lib.check(hip_ops._lib.load().iq_edgeconv_gather(  # noqa: E731
            hip_ops._p(x), hip_ops._p(ei), hip_ops._p(eo), 1, B, 1024, c, 20, hip_ops._stream()), "iq_edgeconv_gather")
        record("get_graph_feature C=%d" % c, [B, 2 * c, 1024, 20], lib_edge, lambda: eager_graph_feature(x, 20, ei64),
               nbytes(eo, ei, x), lambda: hip_ops.edgeconv_gather(x, ei64))

    # PointConv knn_point: 512 queries, 32 neighbours (the eager form returns the set unsorted, this one sorted)
    pc = torch.rand((B, 1024, 3), device=d, generator=g)
    q = pc[:, :512].contiguous()
    record("knn_point", [B, 512, 1024, 32], lambda: hip_ops.knn_point(pc, q, 32),
           lambda: torch.topk(eager_square_distance(q, pc), 32, dim=-1, largest=False, sorted=False)[1])

    # PointConv compute_density
    bw = 0.1
    record("compute_density", [B, 1024], lambda: hip_ops.density(pc, bw),
           lambda: (torch.exp(-eager_square_distance(pc, pc) / (2.0 * bw * bw)) / (2.5 * bw)).mean(dim=-1))

    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "statistic": "median of per-call event times",
              "ops": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    slower = [r["op"] for r in rows if r["speedup"] < 1.0]
    print("kernels slower than eager:", slower or "none")
    print("through the validating wrapper, slower than eager:", [r["op"] for r in rows if r.get("wrapper_speedup", 2) < 1.0] or "none")
    return 1 if slower else 0


if __name__ == "__main__":
    sys.exit(main())
