"""PointNet classifier on the HIP path.

Host-side mirror of models/pointnet.py:91-115 (PointNetCls) of the reference: same constructor
argument, same ``state_dict`` keys (so tools/final_util.py:236-262-style checkpoints load), same
call signature ``model(x: (B,3,N)) -> (logits, trans_feat, crt_points)``.  The arithmetic runs in
libiq_hip.so (csrc/iq_pointnet.hip); the torch modules below only hold parameters.

In addition to the reference's dense ``forward`` the module exposes ``coalition_logits``: the
logits of a batch of region coalitions of one or more clouds WITHOUT materialising the masked
clouds - this is what the Shapley / interaction drivers call.
"""
import ctypes

import numpy as np
import torch
import torch.nn as nn

from . import _lib, hip_ops, workspace
from .engine import Engine, EngineOwner, Packer, check_cloud_of, check_coalition_args, fold, ptr, split_launches, stream


class PackedWeights(Packer):
    """Device-resident, BN-folded, fragment-packed weights + the ctypes struct pointing at them."""

    def __init__(self, state_dict, device):
        super().__init__(device)
        lib, sd = self.lib, state_dict
        self.struct = _lib.PointNetWeights()

        def dense(name, layer, bn, extra_bias=None):
            w, b = fold(sd, layer, bn)
            if extra_bias is not None:   # added in float64 to the bias already rounded to float32, then rounded again
                b = b.astype(np.float32).astype(np.float64) + extra_bias
            cout, cin = w.shape
            wide = cout % 256 == 0 and cin % 32 == 0       # the 1024 -> 512 -> 256 heads (include/iq.h: iq_dense_layer.w_bf3)
            setattr(self.struct, name, self.dense(w, b, bf3=wide))
            if name in ("fstn_c2", "feat_c2", "fstn_c3", "feat_c3"):   # layers 2-3 of the coalition chains
                setattr(self.struct, name + "_bf3", self.bf3(w))

        def in_layer(name, layer, bn):
            w, b = fold(sd, layer, bn)  # (64,3), (64,)
            setattr(self.struct, name, self.dev(np.concatenate([w, b[:, None]], axis=1)).data_ptr())

        in_layer("stn_in", "feat.stn.conv1", "feat.stn.bn1")
        dense("stn_c2", "feat.stn.conv2", "feat.stn.bn2")
        dense("stn_c3", "feat.stn.conv3", "feat.stn.bn3")
        dense("stn_fc1", "feat.stn.fc1", "feat.stn.bn4")
        dense("stn_fc2", "feat.stn.fc2", "feat.stn.bn5")
        dense("stn_fc3", "feat.stn.fc3", None, extra_bias=np.eye(3).reshape(-1))  # + iden, models/pointnet.py:42-45
        in_layer("feat_in", "feat.conv1", "feat.bn1")
        self.feature_transform = "feat.fstn.conv1.weight" in sd
        if self.feature_transform:
            dense("fstn_c1", "feat.fstn.conv1", "feat.fstn.bn1")
            dense("fstn_c2", "feat.fstn.conv2", "feat.fstn.bn2")
            dense("fstn_c3", "feat.fstn.conv3", "feat.fstn.bn3")
            dense("fstn_fc1", "feat.fstn.fc1", "feat.fstn.bn4")
            dense("fstn_fc2", "feat.fstn.fc2", "feat.fstn.bn5")
            # fc3 of the feature STN: output = packed B image of trans_feat (+ identity)
            w3, b3 = fold(sd, "feat.fstn.fc3", None)
        else:   # feature_transform = False: the trunk gets the packed identity (the struct's fstn_c1.w stays NULL)
            w3, b3 = np.zeros((4096, 256)), np.zeros(4096)
        w3 = np.ascontiguousarray(w3, dtype=np.float32)
        b3 = np.ascontiguousarray(b3, dtype=np.float32)
        ow = np.empty(lib.iq_packed_floats(4096, 256), dtype=np.float32)
        ob = np.empty(4096, dtype=np.float32)
        perm = np.empty(4096, dtype=np.int32)
        _lib.check(lib.iq_pack_fstn_fc3(w3.ctypes.data, b3.ctypes.data, ow.ctypes.data, ob.ctypes.data,
                                        perm.ctypes.data), "iq_pack_fstn_fc3")
        wt, bt = self.dev(ow), self.dev(ob)
        self.struct.fstn_fc3 = _lib.DenseLayer(wt.data_ptr(), bt.data_ptr(), 256, 4096)
        inv = np.empty(4096, dtype=np.int64)
        inv[perm] = np.arange(4096)
        self.unpack_index = torch.from_numpy(inv).to(device)  # trans_feat.flatten() = packed[unpack_index]
        dense("feat_c2", "feat.conv2", "feat.bn2")
        dense("feat_c3", "feat.conv3", "feat.bn3")
        dense("cls_fc1", "fc1", "bn1")
        dense("cls_fc2", "fc2", "bn2")
        dense("cls_fc3", "fc3", None)
        self.num_classes = int(sd["fc3.weight"].shape[0])


ORDER_FUSED_MAX = 4096      # kOrderFusedMax of csrc/iq_pointnet.hip: up to here one kernel sorts a batch's launch order, above it four


class PointNetEngine(Engine):
    """Owns packed weights and a growable workspace; issues iq_pointnet_coalitions."""
    packed = PackedWeights

    def coalition_logits(self, clouds, centers, region_id, keep, cloud_of=None, num_regions=None,
                         channel_first=False, return_trans_feat=False, return_crt=False):
        """clouds (nc,N,3) [or (nc,3,N)], centers (nc,3) or None (dense: nothing masked),
        region_id (nc,N) int32, keep (B,) int64 bit masks or None, cloud_of (B,) int32 or None.
        -> logits (B, num_classes) [, packed trans_feat (B,4096)] [, crt_points (B,1024) int32: the point that attains each
        pooled channel's maximum, index N = the centre (iq_pointnet_coalitions_crt)]."""
        nc = clouds.shape[0]
        n = clouds.shape[2] if channel_first else clouds.shape[1]
        b = keep.shape[0] if keep is not None else (cloud_of.shape[0] if cloud_of is not None else nc)
        r = int(num_regions)
        check_coalition_args(clouds, centers, region_id, keep, cloud_of, masked=False)
        logits = self.new_logits(b)
        tfp = torch.empty((b, 4096), dtype=torch.float32, device=self.device) if return_trans_feat else None
        crt = torch.empty((b, 1024), dtype=torch.int32, device=self.device) if return_crt else None
        ws = workspace.ensure(self, self.lib.iq_pointnet_workspace_bytes(b, nc, n, r))
        rc = self.lib.iq_pointnet_coalitions_crt(ctypes.byref(self.weights.struct), ptr(clouds), ptr(centers), ptr(region_id),
                                                 ptr(keep), ptr(cloud_of), ptr(logits), ptr(tfp), ptr(crt), ptr(ws), ws.numel(),
                                                 b, nc, n, r, int(channel_first), stream())
        _lib.check(rc, "iq_pointnet_coalitions")
        out = (logits,) + ((tfp,) if return_trans_feat else ()) + ((crt,) if return_crt else ())
        return out if len(out) > 1 else logits

    def wide_bytes(self, b, nc, n, r):
        return self.lib.iq_pointnet_wide_workspace_bytes(b, nc, n, r)

    def coalition_logits_wide(self, clouds, centers, region_id, keep, cloud_of=None, num_regions=None, return_trans_feat=False):
        """One iq_pointnet_coalitions_wide launch: clouds (nc,N,3), centers (nc,3), region_id (nc,N) int32, keep (B,W) int64 rows of
        W = ceil(num_regions / 64) words, cloud_of (B,) int32 or None -> logits (B, num_classes) [, packed trans_feat (B,4096)].
        Unlike ``coalition_logits`` it takes channel-last clouds only and returns no crt_points (the C entry point has
        channel_first; no wide caller needs it), and centers and keep are required: the dense forward goes through the narrow
        entry."""
        r = int(num_regions)
        hip_ops.wide_words(r)
        check_coalition_args(clouds, centers, region_id, keep, cloud_of)
        hip_ops.wide_keep(keep, r)
        nc, n, b = clouds.shape[0], clouds.shape[1], keep.shape[0]
        logits = self.new_logits(b)
        tfp = torch.empty((b, 4096), dtype=torch.float32, device=self.device) if return_trans_feat else None
        ws = workspace.ensure(self, self.wide_bytes(b, nc, n, r))
        rc = self.lib.iq_pointnet_coalitions_wide(ctypes.byref(self.weights.struct), ptr(clouds), ptr(centers), ptr(region_id),
                                                  ptr(keep), ptr(cloud_of), ptr(logits), ptr(tfp), ptr(ws), ws.numel(),
                                                  b, nc, n, r, 0, stream())
        _lib.check(rc, "iq_pointnet_coalitions_wide")
        return (logits, tfp) if return_trans_feat else logits

    def prefix_logits_wide(self, clouds, centers, region_id, orders, cloud_of=None, num_regions=None, return_trans_feat=False):
        """One iq_pointnet_prefix_coalitions_wide launch: the prefix coalitions of the permutations ``orders`` (S,R) int32 without
        keep rows - row o*(R+1)+i of the result keeps orders[o][:i] - bit for bit ``coalition_logits_wide`` on
        hip_ops.prefix_keep_masks_wide(orders).  clouds (nc,N,3), centers (nc,3), region_id (nc,N) int32; cloud_of (S,) int32 names
        the cloud of each PERMUTATION (required when 1 < nc != S) -> logits (S*(R+1), num_classes) [, packed trans_feat]."""
        r = int(num_regions)
        hip_ops.wide_words(r)
        check_coalition_args(clouds, centers, region_id, None, cloud_of, masked=False)
        if centers is None:
            raise _lib.IqError("centers must be a contiguous %s GPU tensor" % torch.float32)
        if orders.dim() != 2 or orders.shape[1] != r:
            raise _lib.IqError("orders must be (S, %d), got %s" % (r, tuple(orders.shape)))
        op = hip_ops._dev(orders, torch.int32, "orders")
        check_cloud_of(clouds, orders, cloud_of)
        nc, n, s = clouds.shape[0], clouds.shape[1], orders.shape[0]
        b = s * (r + 1)
        logits = self.new_logits(b)
        tfp = torch.empty((b, 4096), dtype=torch.float32, device=self.device) if return_trans_feat else None
        ws = workspace.ensure(self, self.wide_bytes(b, nc, n, r))
        rc = self.lib.iq_pointnet_prefix_coalitions_wide(ctypes.byref(self.weights.struct), ptr(clouds), ptr(centers),
                                                         ptr(region_id), op, ptr(cloud_of), ptr(logits), ptr(tfp), ptr(ws),
                                                         ws.numel(), s, nc, n, r, stream())
        _lib.check(rc, "iq_pointnet_prefix_coalitions_wide")
        return (logits, tfp) if return_trans_feat else logits

    def forward(self, x):
        """Dense forward, x (B,3,N) -> (logits, trans_feat (B,64,64), crt_points (B,1024) int64)."""
        b, _, n = x.shape
        rid = torch.zeros((b, n), dtype=torch.int32, device=self.device)
        logits, tfp, crt = self.coalition_logits(x.contiguous(), None, rid, None, None, num_regions=1,
                                                 channel_first=True, return_trans_feat=True, return_crt=True)
        trans_feat = tfp.index_select(1, self.weights.unpack_index).reshape(b, 64, 64) if self.weights.feature_transform else None
        return logits, trans_feat, crt.long()   # trans_feat is None without a feature STN, as in models/pointnet.py:78


def _param_holder_stn(k):
    m = nn.Module()
    m.conv1, m.conv2, m.conv3 = nn.Conv1d(k, 64, 1), nn.Conv1d(64, 128, 1), nn.Conv1d(128, 1024, 1)
    m.fc1, m.fc2, m.fc3 = nn.Linear(1024, 512), nn.Linear(512, 256), nn.Linear(256, k * k)
    for j, c in enumerate((64, 128, 1024, 512, 256), start=1):
        setattr(m, "bn%d" % j, nn.BatchNorm1d(c))
    return m


class PointNetCls(EngineOwner, nn.Module):
    """Parameter container with the reference's state-dict layout; forward runs on the HIP path."""
    eval_only = "the HIP PointNet path implements eval mode only (BN running stats, no dropout)"

    def __init__(self, args=None):
        super().__init__()
        self.args = args
        dataset = getattr(args, "dataset", "modelnet10")
        self.output_channels = 40 if dataset == "modelnet40" else 10  # models/pointnet.py:95-98
        self.feature_transform = bool(getattr(args, "feature_transform", True))   # models/pointnet.py:99 (the scripts set True)
        feat = nn.Module()
        feat.stn = _param_holder_stn(3)
        feat.conv1, feat.conv2, feat.conv3 = nn.Conv1d(3, 64, 1), nn.Conv1d(64, 128, 1), nn.Conv1d(128, 1024, 1)
        feat.bn1, feat.bn2, feat.bn3 = nn.BatchNorm1d(64), nn.BatchNorm1d(128), nn.BatchNorm1d(1024)
        if self.feature_transform:
            feat.fstn = _param_holder_stn(64)
        self.feat = feat
        self.fc1, self.fc2, self.fc3 = nn.Linear(1024, 512), nn.Linear(512, 256), nn.Linear(256, self.output_channels)
        self.bn1, self.bn2 = nn.BatchNorm1d(512), nn.BatchNorm1d(256)

    def _new_engine(self):
        return PointNetEngine(self.state_dict(), self.fc3.weight.device)

    def forward(self, x):
        """x (B,3,N) -> (logits, trans_feat, crt_points), the reference's tuple (models/pointnet.py:109-115): crt_points (B,1024)
        int64 = the point that attains each pooled channel's maximum (:83), from the arg-max variant of the trunk kernel.
        The coalition path (every hot-path caller discards crt_points, tools/final_common.py:36-37) does not compute it."""
        return self.engine().forward(x)

    def coalition_logits(self, clouds, centers, region_id, keep, cloud_of=None, num_regions=None, validate=True):
        """``validate``: check region_id against [0, num_regions) first (one stream sync); the drivers validate the ids
        once per cloud on the host and pass False."""
        if validate:
            hip_ops.check_index_range(region_id, 0, int(num_regions), "region_id")
        return self.engine().coalition_logits(clouds, centers, region_id, keep, cloud_of, num_regions=num_regions)

    max_wide_per_call = 1 << 16   # coalitions per wide launch: 2 GB of workspace at N = 1024; 1000 permutations of 1024 players are 16 launches

    def coalition_logits_wide(self, clouds, centers, region_id, keep, cloud_of=None, num_regions=None, validate=True):
        """Logits of B WIDE coalitions: ``keep`` (B, ceil(num_regions / 64)) int64 rows, num_regions up to
        hip_ops.MAX_WIDE_REGIONS (one region per point included).  Launches of at most ``max_wide_per_call`` coalitions, fewer when
        the free memory asks for it (engine.split_launches, which the other families' CoalitionModel.split_launches calls too: only
        ``keep`` and ``cloud_of`` are sliced); a coalition's logits do not depend on what else is in its launch."""
        r = int(num_regions)
        hip_ops.wide_words(r)
        if validate:
            hip_ops.check_index_range(region_id, 0, r, "region_id")
        eng = self.engine()
        nc, n = clouds.shape[0], clouds.shape[1]
        return split_launches(eng, lambda k, names: eng.coalition_logits_wide(clouds, centers, region_id, k, names, num_regions=r),
                              lambda k: eng.wide_bytes(k, nc, n, r), self.max_wide_per_call, clouds, keep, cloud_of)

    def prefix_logits_wide(self, clouds, centers, region_id, orders, cloud_of=None, num_regions=None, validate=True):
        """Logits of the prefix coalitions of the permutations ``orders`` (S, num_regions) int32, straight from the permutations:
        row o*(R+1)+i keeps orders[o][:i], ``cloud_of`` (S,) names each permutation's cloud.  Bit for bit
        ``coalition_logits_wide`` on hip_ops.prefix_keep_masks_wide(orders), without the keep rows and with one pass over the
        pre-pooled rows per permutation.  Launches of whole permutations, at most ``max_wide_per_call // (R+1)`` of them (at least
        one), fewer when the free memory asks for it (engine.split_launches slices ``orders`` and ``cloud_of``)."""
        r = int(num_regions)
        hip_ops.wide_words(r)
        if validate:
            hip_ops.check_index_range(region_id, 0, r, "region_id")
        eng = self.engine()
        nc, n = clouds.shape[0], clouds.shape[1]
        return split_launches(eng, lambda o, names: eng.prefix_logits_wide(clouds, centers, region_id, o, names, num_regions=r),
                              lambda k: eng.wide_bytes(k * (r + 1), nc, n, r), max(1, self.max_wide_per_call // (r + 1)), clouds,
                              orders, cloud_of)
