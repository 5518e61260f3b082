"""PointConv (density) classifier on the HIP path.

Host-side mirror of models/pointconv.py:394-424 (PointConvDensityClsSsg): same constructor argument,
same ``state_dict`` keys (226 tensors), same call ``model(xyz: (B,3,N)) -> logits (B,10)``.  Density,
FPS, kNN grouping, the shared MLPs, DensityNet / WeightNet and the weighted aggregation run in
libiq_hip.so (csrc/iq_pointconv.hip); the torch modules only hold parameters.
"""
import ctypes

import numpy as np
import torch
import torch.nn as nn

from . import _lib, hip_ops
from .engine import CoalitionModel, Engine, Packer, check_cloud_of, fold, ptr, stream

SA = [dict(npoint=512, nsample=32, in_channel=3, mlp=[64, 64, 128], bandwidth=0.1),          # models/pointconv.py:403
      dict(npoint=128, nsample=64, in_channel=128 + 3, mlp=[128, 128, 256], bandwidth=0.2),  # :404
      dict(npoint=1, nsample=None, in_channel=256 + 3, mlp=[256, 512, 1024], bandwidth=0.4)]  # :405


class PackedWeightsC(Packer):
    def __init__(self, sd, device):
        super().__init__(device)
        self.struct = _lib.PointConvWeights()
        dev, bf3 = self.dev, self.bf3

        def dense(w, b):
            cout, cin = w.shape
            return self.dense(w, b, bf3=cout % 256 == 0 and cin >= 32)    # wide layers: also as three bf16 terms (include/iq.h)

        def tiny(prefix):
            rows = []
            for j in range(3):
                w, b = fold(sd, "%s.mlp_convs.%d" % (prefix, j), "%s.mlp_bns.%d" % (prefix, j))
                rows.append(np.concatenate([w, b[:, None]], axis=1).reshape(-1))
            return dev(np.concatenate(rows)).data_ptr()

        for k, cfg in enumerate(SA):
            p = "sa%d" % (k + 1)
            dst = self.struct.sa[k]
            w0, b0 = fold(sd, p + ".mlp_convs.0", p + ".mlp_bns.0")
            feat = cfg["in_channel"] - 3                               # input = [x_p - c (3) ; features]  (:133-135)
            bias = b0 if feat == 0 else np.zeros_like(b0)
            dst.w1x = dev(np.concatenate([w0[:, :3], bias[:, None]], axis=1)).data_ptr()
            if feat:
                dst.u = dense(w0[:, 3:], b0)
            w2, b2 = fold(sd, p + ".mlp_convs.1", p + ".mlp_bns.1")
            w3, b3 = fold(sd, p + ".mlp_convs.2", p + ".mlp_bns.2")
            dst.l2, dst.l3 = dense(w2, b2), dense(w3, b3)
            if k == 1 and w2.shape == (128, 128) and w3.shape == (256, 128):   # sa2's grouped MLP on the bf16 matrix pipe
                self.struct.sa2_l2_bf3, self.struct.sa2_l3_bf3 = bf3(w2), bf3(w3)
            dst.densitynet = tiny(p + ".densitynet")
            dst.weightnet = tiny(p + ".weightnet")
            dst.linear = dense(*fold(sd, p + ".linear", p + ".bn_linear"))
            dst.bandwidth = cfg["bandwidth"]
            dst.nsample = cfg["nsample"] or 0
        self.struct.fc1 = dense(*fold(sd, "fc1", "bn1"))
        self.struct.fc2 = dense(*fold(sd, "fc2", "bn2"))
        self.struct.fc3 = dense(*fold(sd, "fc3", None))
        self.num_classes = int(sd["fc3.weight"].shape[0])


class PointConvEngine(Engine):
    packed = PackedWeightsC
    forward_name, coalitions_name = "iq_pointconv_forward", "iq_pointconv_coalitions"

    def __init__(self, state_dict, device):
        super().__init__(state_dict, device)
        self._tab = {}      # which source clouds the tables at the head of the workspace belong to (_tables_state)

    def workspace_replaced(self):
        self._tab = {}              # whatever the old workspace cached (the per-cloud tables) is gone

    def forward_bytes(self, b, n):
        return self.lib.iq_pointconv_workspace_bytes(b, n)

    def _forward(self, xyz, logits, ws, b, n):
        self._tab = {}              # the dense forward's arrays start at the head of the workspace, where the coalition path keeps its tables
        return self.lib.iq_pointconv_forward(ctypes.byref(self.weights.struct), ptr(xyz), ptr(logits), ptr(ws), ws.numel(), b, n, stream())

    def coalition_bytes(self, b, nc, n):
        return self.lib.iq_pointconv_coalitions_workspace_bytes(b, nc, n)

    def _coalitions(self, clouds, centers, region_id, keep, cloud_of, logits, ws, b, nc, n, walk=None):
        """The masked clouds are written inside the library; sa1 / sa2 groups from the source clouds' sorted neighbour lists
        (csrc/iq_pointconv.hip).  walk: True / False names how groups are formed (sorted-list walk or a kNN per coalition) for a
        batch that is split over several launches; None lets the library decide from this launch alone."""
        state = ctypes.c_int(self._tables_state(clouds, centers, nc, n) | (0 if walk is None else (4 if walk else 8)))
        rc = self.lib.iq_pointconv_coalitions_cached(ctypes.byref(self.weights.struct), ptr(clouds), ptr(centers), ptr(region_id), ptr(keep),
                                                     ptr(cloud_of), ptr(logits), ptr(ws), ws.numel(), b, nc, n, ctypes.byref(state), stream())
        if rc == 0:
            self._tab["state"] = state.value & 3
        return rc

    def _coalitions_wide(self, clouds, centers, region_id, keep, cloud_of, logits, ws, b, nc, n, r, walk=None):
        """``_coalitions`` for wide keep rows: the same cached tables (they belong to the source clouds, not to the masks)."""
        state = ctypes.c_int(self._tables_state(clouds, centers, nc, n) | (0 if walk is None else (4 if walk else 8)))
        rc = self.lib.iq_pointconv_coalitions_cached_wide(ctypes.byref(self.weights.struct), ptr(clouds), ptr(centers), ptr(region_id),
                                                          ptr(keep), ptr(cloud_of), ptr(logits), ptr(ws), ws.numel(), b, nc, n,
                                                          ctypes.byref(state), r, stream())
        if rc == 0:
            self._tab["state"] = state.value & 3
        return rc

    def _tables_state(self, clouds, centers, nc, n):
        """Which per-cloud structures (sorted lists, sa1 pair tables) the head of the workspace still holds for THESE clouds:
        the same workspace allocation, the same (nc, N), and the same `clouds` / `centers` TENSORS at the same version (torch
        counts every in-place write) as the call that built them - an identity test, no read-back, no synchronisation (comparing
        the coordinates on the device cost a host sync per launch: 4.8 ms of exposed launch latency per 3300-coalition step).
        The two tensors are held, so their memory cannot be handed to other data meanwhile.  The launches of one driver call
        (the chunks of an interaction ratio, the batches of a pose) pass the same tensors and re-use the tables; round 3 rebuilt
        ~1 GB per source cloud on every launch.  (Writing into a held tensor behind torch's back - a raw pointer - is not seen.)"""
        t = self._tab
        try:
            versions = (clouds._version, centers._version)
        except RuntimeError:        # inference tensors carry no version counter: nothing to tell a rewrite by, so rebuild
            self._tab = {}
            return 0
        # the stream is part of the key: tables another stream is still building must not be read from this one
        key = (self._ws.data_ptr(), nc, n, clouds.data_ptr(), centers.data_ptr(), versions, torch.cuda.current_stream().cuda_stream)
        if t.get("key") == key and t.get("state", 0) and t["clouds"] is clouds and t["centers"] is centers:
            return int(t["state"])
        self._tab = {"key": key, "clouds": clouds, "centers": centers, "state": 0}
        return 0


def _tiny_holder(dims):
    m = nn.Module()
    m.mlp_convs, m.mlp_bns = nn.ModuleList(), nn.ModuleList()
    for j in range(3):
        m.mlp_convs.append(nn.Conv2d(dims[j], dims[j + 1], 1))
        m.mlp_bns.append(nn.BatchNorm2d(dims[j + 1]))
    return m


def _sa_holder(cfg):
    m = nn.Module()
    m.mlp_convs, m.mlp_bns = nn.ModuleList(), nn.ModuleList()
    last = cfg["in_channel"]
    for c in cfg["mlp"]:
        m.mlp_convs.append(nn.Conv2d(last, c, 1))
        m.mlp_bns.append(nn.BatchNorm2d(c))
        last = c
    m.weightnet = _tiny_holder([3, 8, 8, 16])
    m.linear = nn.Linear(16 * last, last)
    m.bn_linear = nn.BatchNorm1d(last)
    m.densitynet = _tiny_holder([1, 16, 8, 1])
    return m


class PointConvDensityClsSsg(CoalitionModel, nn.Module):
    """Parameter container with the reference's state-dict layout; forward runs on the HIP path."""
    eval_only = "the HIP PointConv path implements eval mode only"

    max_clouds_per_call = 4096  # bounds the workspace (9.5 MB per cloud: 39 GB of the 288 GB; one launch covers a 3300-coalition pose)
    preferred_clouds_per_call = 4096  # drivers batch at least this many materialised clouds per launch

    def __init__(self, args=None):
        super().__init__()
        self.args = args
        self.output_channels = 40 if getattr(args, "dataset", "modelnet10") == "modelnet40" else 10
        self.sa1, self.sa2, self.sa3 = _sa_holder(SA[0]), _sa_holder(SA[1]), _sa_holder(SA[2])
        self.fc1, self.bn1 = nn.Linear(1024, 512), nn.BatchNorm1d(512)
        self.fc2, self.bn2 = nn.Linear(512, 256), nn.BatchNorm1d(256)
        self.fc3 = nn.Linear(256, self.output_channels)

    def _new_engine(self):
        return PointConvEngine(self.state_dict(), self.fc3.weight.device)

    def split_launches(self, eng, clouds, centers, region_id, keep, cloud_of):
        """Clouds of more than 1024 points go through mask kernel + forward_points, source cloud by source cloud; fewer than 64
        points are rejected here as in the dense forward (sa2 groups 64 neighbours; below 512 points sa1's sampling repeats
        index 0, as models/pointconv.py:54-77 does)."""
        nc, b = clouds.shape[0], keep.shape[0]
        if clouds.shape[1] < 64:
            raise _lib.IqError("PointConv needs at least 64 points per cloud (sa2 groups 64 neighbours), got %d" % clouds.shape[1])
        if clouds.shape[1] > 1024:   # beyond the library's coalition entry: mask kernel + forward, source cloud by source cloud
            check_cloud_of(clouds, keep, cloud_of)
            which = cloud_of if cloud_of is not None else (torch.zeros(b, dtype=torch.int32, device=keep.device) if nc == 1
                                                          else torch.arange(b, dtype=torch.int32, device=keep.device))
            out = torch.empty((b, self.output_channels), dtype=torch.float32, device=keep.device)
            for c in range(nc):
                sel = torch.nonzero(which == c).flatten()
                if sel.numel():
                    x = hip_ops.mask_coalitions(clouds[c].contiguous(), region_id[c].contiguous(), keep[sel].contiguous(),
                                                centers[c].contiguous())
                    out[sel] = self.forward_points(x)
            return out
        # how groups are formed is decided ONCE, from the whole batch (the library's own rule, iq.h): a memory-tight run that splits
        # the batch - or its short last launch - must not switch to the other summation order
        return super().split_launches(eng, clouds, centers, region_id, keep, cloud_of, nc <= 8 or nc * 8 <= b)

    def split_launches_wide(self, eng, clouds, centers, region_id, keep, cloud_of, r):
        """The compact path takes clouds of 64 to 1024 points; there is no dense detour here (wide.py's "dense" route is one).  How
        groups are formed is decided once from the whole batch, as in ``split_launches``."""
        nc, b, n = clouds.shape[0], keep.shape[0], clouds.shape[1]
        if not 64 <= n <= 1024:
            raise _lib.IqError("PointConv's compact coalition path takes clouds of 64 to 1024 points, got %d" % n)
        return super().split_launches_wide(eng, clouds, centers, region_id, keep, cloud_of, r, nc <= 8 or nc * 8 <= b)
