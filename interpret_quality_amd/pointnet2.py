"""PointNet++ MSG classifier on the HIP path.

Host-side mirror of models/pointnet2.py:244-276 (PointNet2ClsMsg): same constructor argument, same
``state_dict`` keys (163 tensors), same call ``model(xyz: (B,3,N)) -> logits (B,10)``.  The torch
modules only hold parameters; FPS, ball query, grouping, the shared MLPs and the pooling run in
libiq_hip.so (csrc/iq_pointnet2.hip, iq_geom.hip).
"""
import ctypes

import numpy as np
import torch.nn as nn

from . import _lib
from .engine import CoalitionModel, Engine, Packer, fold, ptr, stream

SA1 = dict(npoint=512, radius=[0.1, 0.2, 0.4], nsample=[16, 32, 128], in_channel=0,
           mlp=[[32, 32, 64], [64, 64, 128], [64, 96, 128]])                         # models/pointnet2.py:253
SA2 = dict(npoint=128, radius=[0.2, 0.4, 0.8], nsample=[32, 64, 128], in_channel=320,
           mlp=[[64, 64, 128], [128, 128, 256], [128, 128, 256]])                    # :254
SA3_MLP = [256, 512, 1024]                                                           # :255


class PackedWeights2(Packer):
    def __init__(self, sd, device):
        super().__init__(device)
        self.struct = _lib.PointNet2Weights()
        dev, bf3 = self.dev, self.bf3

        def dense(w, b):
            cout, cin = w.shape
            # wide layers: also as three bf16 terms (include/iq.h); 320 outputs: the first 256 columns take them
            return self.dense(w, b, bf3=(cout % 256 == 0 or (cout > 256 and cout % 256 == 64)) and cin >= 32)

        def scale(dst, sa, i, cfg, feat_in):
            w0, b0 = fold(sd, "%s.conv_blocks.%d.0" % (sa, i), "%s.bn_blocks.%d.0" % (sa, i))
            wx = w0[:, feat_in:feat_in + 3]                       # relative xyz comes LAST (models/pointnet2.py:226)
            bias = b0 if feat_in == 0 else np.zeros_like(b0)      # with features the bias travels in U
            dst.w1x = dev(np.concatenate([wx, bias[:, None]], axis=1)).data_ptr()
            w2, b2 = fold(sd, "%s.conv_blocks.%d.1" % (sa, i), "%s.bn_blocks.%d.1" % (sa, i))
            w3, b3 = fold(sd, "%s.conv_blocks.%d.2" % (sa, i), "%s.bn_blocks.%d.2" % (sa, i))
            dst.l2, dst.l3 = dense(w2, b2), dense(w3, b3)
            if sa == "sa2" and w2.shape == (128, 128) and w3.shape == (256, 128):   # the widest scales: bf16 matrix pipe
                self.struct.sa2_l2_bf3[i], self.struct.sa2_l3_bf3[i] = bf3(w2), bf3(w3)
            dst.radius = cfg["radius"][i]
            dst.nsample = cfg["nsample"][i]
            return w0[:, :feat_in], b0

        for i in range(3):
            scale(self.struct.sa1[i], "sa1", i, SA1, 0)
        uw, ub = [], []
        for i in range(3):
            wf, b0 = scale(self.struct.sa2[i], "sa2", i, SA2, 320)
            uw.append(wf)
            ub.append(b0)
        self.struct.sa2_u = dense(np.concatenate(uw, axis=0), np.concatenate(ub, axis=0))
        w, b = fold(sd, "sa3.mlp_convs.0", "sa3.mlp_bns.0")   # input = [xyz, features] (xyz FIRST, :132-135)
        wpad = np.zeros((w.shape[0], 648))
        wpad[:, :643] = w
        self.struct.sa3_l1 = dense(wpad, b)
        self.struct.sa3_l2 = dense(*fold(sd, "sa3.mlp_convs.1", "sa3.mlp_bns.1"))
        self.struct.sa3_l3 = dense(*fold(sd, "sa3.mlp_convs.2", "sa3.mlp_bns.2"))
        self.struct.fc1 = dense(*fold(sd, "fc1", "bn1"))
        self.struct.fc2 = dense(*fold(sd, "fc2", "bn2"))
        self.struct.fc3 = dense(*fold(sd, "fc3", None))
        self.num_classes = int(sd["fc3.weight"].shape[0])


class PointNet2Engine(Engine):
    packed = PackedWeights2
    forward_name, coalitions_name = "iq_pointnet2_forward", "iq_pointnet2_coalitions"

    def forward_bytes(self, b, n):
        return self.lib.iq_pointnet2_workspace_bytes(b)

    def _forward(self, xyz, logits, ws, b, n):
        return self.lib.iq_pointnet2_forward(ctypes.byref(self.weights.struct), ptr(xyz), ptr(logits), ptr(ws), ws.numel(), b, n, stream())

    def coalition_bytes(self, b, nc, n):
        return self.lib.iq_pointnet2_coalitions_workspace_bytes(b, nc, n)

    def _coalitions(self, clouds, centers, region_id, keep, cloud_of, logits, ws, b, nc, n):
        """sa1 from the per-cloud pair tables (csrc/iq_pointnet2.hip)"""
        return self.lib.iq_pointnet2_coalitions(ctypes.byref(self.weights.struct), ptr(clouds), ptr(centers), ptr(region_id), ptr(keep),
                                                ptr(cloud_of), ptr(logits), ptr(ws), ws.numel(), b, nc, n, stream())

    def _coalitions_wide(self, clouds, centers, region_id, keep, cloud_of, logits, ws, b, nc, n, r):
        """sa1 from the per-cloud pair tables by the member walk; clouds of at most 1024 points"""
        return self.lib.iq_pointnet2_coalitions_wide(ctypes.byref(self.weights.struct), ptr(clouds), ptr(centers), ptr(region_id),
                                                     ptr(keep), ptr(cloud_of), ptr(logits), ptr(ws), ws.numel(), b, nc, n, r, stream())


def _holder_msg(cfg):
    m = nn.Module()
    m.conv_blocks, m.bn_blocks = nn.ModuleList(), nn.ModuleList()
    for mlp in cfg["mlp"]:
        convs, bns = nn.ModuleList(), nn.ModuleList()
        last = cfg["in_channel"] + 3
        for c in mlp:
            convs.append(nn.Conv2d(last, c, 1))
            bns.append(nn.BatchNorm2d(c))
            last = c
        m.conv_blocks.append(convs)
        m.bn_blocks.append(bns)
    return m


class PointNet2ClsMsg(CoalitionModel, nn.Module):
    """Parameter container with the reference's state-dict layout; forward runs on the HIP path."""
    eval_only = "the HIP PointNet++ path implements eval mode only"

    max_clouds_per_call = 4096  # bounds the workspace (3.2 MB per cloud: 13 GB; one launch covers a 3300-coalition pose)
    preferred_clouds_per_call = 1024  # drivers batch at least this many materialised clouds per launch

    def __init__(self, args=None):
        super().__init__()
        self.args = args
        self.output_channels = 40 if getattr(args, "dataset", "modelnet10") == "modelnet40" else 10
        self.sa1, self.sa2 = _holder_msg(SA1), _holder_msg(SA2)
        sa3 = nn.Module()
        sa3.mlp_convs, sa3.mlp_bns = nn.ModuleList(), nn.ModuleList()
        last = 640 + 3
        for c in SA3_MLP:
            sa3.mlp_convs.append(nn.Conv2d(last, c, 1))
            sa3.mlp_bns.append(nn.BatchNorm2d(c))
            last = c
        self.sa3 = sa3
        self.fc1, self.bn1 = nn.Linear(1024, 512), nn.BatchNorm1d(512)
        self.fc2, self.bn2 = nn.Linear(512, 256), nn.BatchNorm1d(256)
        self.fc3 = nn.Linear(256, self.output_channels)

    def _new_engine(self):
        return PointNet2Engine(self.state_dict(), self.fc3.weight.device)
