"""DGCNN and GCNN classifiers on the HIP path.

Host-side mirror of models/dgcnn.py:51-194 (DGCNN_cls: dynamic feature-space kNN graph per layer;
GCNN_cls: one fixed xyz graph): same constructor argument, same ``state_dict`` keys (70 tensors, the
BatchNorms appear twice as ``bnK.*`` and ``convK.1.*``), same call ``model(x: (B,3,N)) -> logits``.
kNN, the EdgeConv GEMMs, the neighbour max, conv5, pooling and the head run in libiq_hip.so
(csrc/iq_dgcnn.hip); the torch modules only hold parameters.  ``gcnn_adv`` is GCNN_cls with another
checkpoint (tools/final_util.py:243-244).
"""
import ctypes

import numpy as np
import torch.nn as nn

from . import _lib
from .engine import CoalitionModel, Engine, Packer, _np, bn_affine, ptr, stream

CONVS = [(6, 64), (128, 64), (128, 128), (256, 256)]  # models/dgcnn.py:66-77


class PackedWeightsD(Packer):
    def __init__(self, sd, device, k):
        super().__init__(device)
        self.struct = _lib.DgcnnWeights()
        dense = self.dense      # no layer's w_bf3 is filled, the 2048 -> 512 head included: only conv5_bf3 below

        for j, (cin2, cout) in enumerate(CONVS, start=1):
            c = cin2 // 2
            w = _np(sd["conv%d.0.weight" % j]).reshape(cout, cin2)
            s, t = bn_affine(sd, "bn%d" % j)
            wa, wb = w[:, :c], w[:, c:]                       # [x_j - x_i ; x_i]  (models/dgcnn.py:45)
            cpad = 8 if c == 3 else c
            pq = np.zeros((2 * cout, cpad))
            pq[:cout, :c] = wa * s[:, None]                   # P = (s.W_a) x
            pq[cout:, :c] = (wb - wa) * s[:, None]            # Q = (s.(W_b - W_a)) x + t
            self.struct.pq[j - 1] = dense(pq, np.concatenate([np.zeros(cout), t]))
        s, t = bn_affine(sd, "bn5")
        w5 = _np(sd["conv5.0.weight"]).reshape(1024, 512) * s[:, None]
        self.struct.conv5 = dense(w5, t)
        # conv5 (half of a DGCNN step, three quarters of GCNN's) runs on the bf16 matrix pipe: the same folded float32 weights as
        # three bf16 terms (csrc/iq_linear.hip: pn_gemm_bf3_kernel<pool>)
        self.struct.reserved = 0
        self.struct.conv5_bf3 = self.bf3(w5)
        s, t = bn_affine(sd, "bn6")
        self.struct.fc1 = dense(_np(sd["linear1.weight"]) * s[:, None], t)      # linear1 has no bias (:79)
        s, t = bn_affine(sd, "bn7")
        self.struct.fc2 = dense(_np(sd["linear2.weight"]) * s[:, None], _np(sd["linear2.bias"]) * s + t)
        self.struct.fc3 = dense(_np(sd["linear3.weight"]), _np(sd["linear3.bias"]))
        self.struct.k = k
        self.num_classes = int(sd["linear3.weight"].shape[0])


class DgcnnEngine(Engine):
    packed = PackedWeightsD
    forward_name, coalitions_name = "iq_dgcnn_forward", "iq_dgcnn_coalitions"

    def __init__(self, state_dict, device, k, fixed_graph):
        super().__init__(state_dict, device, k)
        self.fixed_graph = int(fixed_graph)

    def forward_bytes(self, b, n):
        return self.lib.iq_dgcnn_workspace_bytes(b, n)

    def _forward(self, xyz, logits, ws, b, n):
        return self.lib.iq_dgcnn_forward(ctypes.byref(self.weights.struct), ptr(xyz), ptr(logits), ptr(ws), ws.numel(), b, n,
                                         self.fixed_graph, stream())

    def coalition_bytes(self, b, nc, n):
        return self.lib.iq_dgcnn_workspace_bytes(b, n)

    def _coalitions(self, clouds, centers, region_id, keep, cloud_of, logits, ws, b, nc, n):
        """The masked clouds are never written."""
        return self.lib.iq_dgcnn_coalitions(ctypes.byref(self.weights.struct), ptr(clouds), ptr(centers), ptr(region_id), ptr(keep),
                                            ptr(cloud_of), ptr(logits), ptr(ws), ws.numel(), b, nc, n, self.fixed_graph, stream())

    def _coalitions_wide(self, clouds, centers, region_id, keep, cloud_of, logits, ws, b, nc, n, r):
        return self.lib.iq_dgcnn_coalitions_wide(ctypes.byref(self.weights.struct), ptr(clouds), ptr(centers), ptr(region_id),
                                                 ptr(keep), ptr(cloud_of), ptr(logits), ptr(ws), ws.numel(), b, nc, n,
                                                 self.fixed_graph, r, stream())


class _GraphCnn(CoalitionModel, nn.Module):
    fixed_graph = False
    eval_only = "the HIP DGCNN path implements eval mode only"
    max_clouds_per_call = 4096  # bounds the workspace (4.4 MB per cloud)

    def __init__(self, args=None):
        super().__init__()
        self.args = args
        self.k = getattr(args, "k", 20)
        self.output_channels = 40 if getattr(args, "dataset", "modelnet10") == "modelnet40" else 10
        self.bn1, self.bn2, self.bn3, self.bn4 = nn.BatchNorm2d(64), nn.BatchNorm2d(64), nn.BatchNorm2d(128), nn.BatchNorm2d(256)
        self.bn5 = nn.BatchNorm1d(1024)
        for j, (cin, cout) in enumerate(CONVS, start=1):
            setattr(self, "conv%d" % j, nn.Sequential(nn.Conv2d(cin, cout, kernel_size=1, bias=False),
                                                     getattr(self, "bn%d" % j), nn.LeakyReLU(negative_slope=0.2)))
        self.conv5 = nn.Sequential(nn.Conv1d(512, 1024, kernel_size=1, bias=False), self.bn5, nn.LeakyReLU(negative_slope=0.2))
        self.linear1 = nn.Linear(2048, 512, bias=False)
        self.bn6 = nn.BatchNorm1d(512)
        self.linear2 = nn.Linear(512, 256)
        self.bn7 = nn.BatchNorm1d(256)
        self.linear3 = nn.Linear(256, self.output_channels)

    def _new_engine(self):
        return DgcnnEngine(self.state_dict(), self.linear3.weight.device, self.k, self.fixed_graph)


class DGCNN_cls(_GraphCnn):
    """models/dgcnn.py:51-120."""
    fixed_graph = False


class GCNN_cls(_GraphCnn):
    """models/dgcnn.py:123-194."""
    fixed_graph = True
