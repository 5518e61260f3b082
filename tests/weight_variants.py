"""Stress variants of the synthetic weights: pure functions from a reference-keyed numpy state dict (what
``synth.*_state_dict(seed)`` returns) to a new dict of the same keys, shapes and dtypes.  ``synth`` itself is untouched: the
goldens depend on what it returns for every seed.

Importing this module touches no GPU and no torch.  Not collected by pytest (no test_ prefix).

* ``rescaled``: every eligible BatchNorm's ``weight`` and ``bias`` times 2^k[c], the columns that read channel c in every
  following layer divided by the same 2^k[c].  The network is the same function, and the same bits in any float32
  implementation whose summation order does not depend on values: a power-of-two factor commutes with rounding, ReLU,
  LeakyReLU, max and sums (no overflow or underflow at these magnitudes).
* ``dead_channels``: gamma = 0 on a fraction of every BatchNorm's channels, their bias < 0, > 0, +0.0 or -0.0.
* ``negative_shift``: every bias in front of a (Leaky)ReLU lowered, so most activations are exactly 0 (negative under LeakyReLU).
* ``variance_spread``: running variances log-uniform over a range.

Which BatchNorms ``rescaled`` covers (``rescale_plan``), by family:

* pointnet: both STNs' bn1 - bn5, feat.bn2, feat.bn3, head bn1 and bn2 (14).  Not feat.bn1 (it feeds the feature STN and, through
  the regressed 64 x 64 transform, conv2) and nothing behind an STN's fc3 (its output is the transform itself).
* pointnet2: all 18 BatchNorms of sa1 / sa2 (the last layer of each scale goes, through the max over the group and the concatenation
  [scale 0, scale 1, scale 2], into sa2's first layers - features first, relative xyz last - and into sa3's first layer - xyz
  first), sa3's three, head bn1 and bn2 (23).
* pointconv: per stage the grouped MLP's three layers (the last one reaches ``linear`` as column c * 16 + j), WeightNet's three
  (channel j of the last: columns j, 16 + j, ...), DensityNet's three (the last has one channel: every column of ``linear``),
  ``bn_linear`` (next stage's first layer after the 3 xyz columns; sa3's: fc1); head bn1 and bn2 (32).
* gcnn (one fixed xyz graph): bn1 - bn7 (7): layer l's channel c is read by the next EdgeConv as columns c (x_j - x_i) and C + c
  (x_i) and by conv5 through the concatenation (x1, x2, x3, x4); bn5's by linear1 as c (max pool) and 1024 + c (mean pool).
* dgcnn: bn5, bn6, bn7 only (3): bn1 - bn4 feed the feature-space kNN, and scaling a channel changes the neighbour sets.
"""
import re

import numpy as np

FAMILIES = ("pointnet", "pointnet2", "pointconv", "gcnn", "dgcnn")
PN2_MLPS = {"sa1": [[32, 32, 64], [64, 64, 128], [64, 96, 128]], "sa2": [[64, 64, 128], [128, 128, 256], [128, 128, 256]]}
_DGCNN_ALIAS = re.compile(r"^conv(\d)\.1\.(.*)$")      # the Sequential's BatchNorm is bnK itself (synth.dgcnn_state_dict)


def _copy(sd):
    return {k: np.array(v, copy=True) for k, v in sd.items()}


def _sync_aliases(sd):
    for k in sd:
        m = _DGCNN_ALIAS.match(k)
        if m:
            sd[k] = sd["bn%s.%s" % (m.group(1), m.group(2))]
    return sd


def bn_names(sd):
    """Every BatchNorm of a state dict once (DGCNN's convK.1.* aliases of bnK.* are left out), in key order."""
    return [k[:-len(".running_var")] for k in sd if k.endswith(".running_var") and not _DGCNN_ALIAS.match(k)]


def relu_bn_names(sd, family):
    """The BatchNorms in front of a ReLU or LeakyReLU: all but PointNet's feat.bn3, which goes straight into the max."""
    return [b for b in bn_names(sd) if not (family == "pointnet" and b == "feat.bn3")]


# ---- rescaled ------------------------------------------------------------------------------------------------------------

def _plain(c, off=0):
    return (off + np.arange(c)).reshape(c, 1)


def rescale_plan(family):
    """[(bn name, [(weight key, columns (C, m) int: the input columns of that weight that read channel c)])]."""
    plan = []
    if family == "pointnet":
        for p in ("feat.stn", "feat.fstn"):
            for j, (c, nxt) in enumerate(zip((64, 128, 1024, 512, 256), ("conv2", "conv3", "fc1", "fc2", "fc3")), start=1):
                plan.append(("%s.bn%d" % (p, j), [("%s.%s.weight" % (p, nxt), _plain(c))]))
        plan += [("feat.bn2", [("feat.conv3.weight", _plain(128))]), ("feat.bn3", [("fc1.weight", _plain(1024))])]
    elif family == "pointnet2":
        for sa, nxt, xyz_first in (("sa1", ["sa2.conv_blocks.%d.0.weight" % m for m in range(3)], 0), ("sa2", ["sa3.mlp_convs.0.weight"], 3)):
            off = 0
            for i, mlp in enumerate(PN2_MLPS[sa]):
                for j in (0, 1):
                    plan.append(("%s.bn_blocks.%d.%d" % (sa, i, j), [("%s.conv_blocks.%d.%d.weight" % (sa, i, j + 1), _plain(mlp[j]))]))
                plan.append(("%s.bn_blocks.%d.2" % (sa, i), [(k, _plain(mlp[2], xyz_first + off)) for k in nxt]))
                off += mlp[2]
        for j, (c, nxt) in enumerate(zip((256, 512, 1024), ("sa3.mlp_convs.1", "sa3.mlp_convs.2", "fc1"))):
            plan.append(("sa3.mlp_bns.%d" % j, [(nxt + ".weight", _plain(c))]))
    elif family == "pointconv":
        for k, (mlp, nxt) in enumerate(zip(([64, 64, 128], [128, 128, 256], [256, 512, 1024]),
                                           ("sa2.mlp_convs.0.weight", "sa3.mlp_convs.0.weight", "fc1.weight")), start=1):
            p, last = "sa%d" % k, mlp[2]
            lin = p + ".linear.weight"                                      # input column c * 16 + j: (channel c, WeightNet output j)
            for j in (0, 1):
                plan.append(("%s.mlp_bns.%d" % (p, j), [("%s.mlp_convs.%d.weight" % (p, j + 1), _plain(mlp[j]))]))
            plan.append((p + ".mlp_bns.2", [(lin, np.arange(16 * last).reshape(last, 16))]))
            for net, dims in (("weightnet", [8, 8, 16]), ("densitynet", [16, 8, 1])):
                for j in (0, 1):
                    plan.append(("%s.%s.mlp_bns.%d" % (p, net, j), [("%s.%s.mlp_convs.%d.weight" % (p, net, j + 1), _plain(dims[j]))]))
            plan.append((p + ".weightnet.mlp_bns.2", [(lin, np.arange(16 * last).reshape(last, 16).T.copy())]))
            plan.append((p + ".densitynet.mlp_bns.2", [(lin, np.arange(16 * last).reshape(1, -1))]))
            plan.append((p + ".bn_linear", [(nxt, _plain(last, 0 if k == 3 else 3))]))
    elif family in ("gcnn", "dgcnn"):
        chans, off = (64, 64, 128, 256), (0, 64, 128, 256)
        if family == "gcnn":
            for l in range(4):
                c = chans[l]
                readers = [("conv5.0.weight", _plain(c, off[l]))]
                if l < 3:
                    readers.append(("conv%d.0.weight" % (l + 2), np.stack([np.arange(c), c + np.arange(c)], axis=1)))
                plan.append(("bn%d" % (l + 1), readers))
        plan.append(("bn5", [("linear1.weight", np.stack([np.arange(1024), 1024 + np.arange(1024)], axis=1))]))
        plan += [("bn6", [("linear2.weight", _plain(512))]), ("bn7", [("linear3.weight", _plain(256))])]
        return plan
    else:
        raise ValueError(family)
    plan += [("bn1", [("fc2.weight", _plain(512))]), ("bn2", [("fc3.weight", _plain(256))])]
    return plan


def rescaled(sd, family, kmax, seed, skip_compensation=()):
    """-> (new state dict, names of the BatchNorms scaled).  ``skip_compensation``: BatchNorms whose readers are left as they
    are - a deliberately WRONG rescaling, for the tests that show the invariance check can fail."""
    out = _copy(sd)
    rng = np.random.default_rng([seed, kmax])
    done = []
    for bn, readers in rescale_plan(family):
        c = out[bn + ".weight"].shape[0]
        f = np.exp2(rng.integers(-kmax, kmax + 1, size=c)).astype(np.float32)
        for key in (".weight", ".bias"):
            out[bn + key] = out[bn + key] * f
        done.append(bn)
        if bn in skip_compensation:
            continue
        for key, cols in readers:
            w = out[key]
            assert cols.shape[0] == c and cols.max() < w.shape[1], (bn, key, cols.shape, w.shape)
            div = np.ones(w.shape[1], dtype=np.float32)
            assert np.unique(cols).size == cols.size, (bn, key)
            div[cols] = f[:, None]
            out[key] = w / div.reshape((1, -1) + (1,) * (w.ndim - 2))
    for k in sd:
        assert out[k].dtype == sd[k].dtype and out[k].shape == sd[k].shape, k
    return _sync_aliases(out), done


# ---- dead channels, negative shift, variance spread ----------------------------------------------------------------------------

def dead_channels(sd, frac=1 / 8, seed=0):
    """gamma = 0 on round(frac * C) random channels of every BatchNorm; of those the bias is < 0 for half, > 0 for a quarter, +0.0
    for an eighth and -0.0 for an eighth (in that order of precedence when there are fewer than eight).
    -> (new state dict, {bn name: indices of its dead channels})."""
    out = _copy(sd)
    dead = {}
    for bn in bn_names(sd):
        rng = np.random.default_rng([seed, len(dead)])
        c = out[bn + ".weight"].shape[0]
        idx = rng.permutation(c)[:int(round(frac * c))]
        n = len(idx)
        mag = rng.uniform(0.05, 0.5, size=n).astype(np.float32)
        bias = np.where(np.arange(n) % 2 == 0, -mag, mag)                    # of every eight: 0, 2, 4, 6 negative; 1, 5 positive
        bias[np.arange(n) % 8 == 3] = 0.0                                    # 3: +0.0
        bias[np.arange(n) % 8 == 7] = -0.0                                   # 7: -0.0
        out[bn + ".weight"][idx] = 0.0
        out[bn + ".bias"][idx] = bias.astype(np.float32)
        dead[bn] = idx
    return _sync_aliases(out), dead


# PointConv's WeightNet and DensityNet multiply every channel of their stage: with their biases lowered too the whole network is
# the constant fc3(relu(..)) of zeros, which tests nothing
def _gates_everything(bn):
    return ".weightnet." in bn or ".densitynet." in bn


def negative_shift(sd, family, shift):
    """``shift`` subtracted from the bias of every BatchNorm in front of a ReLU / LeakyReLU (PointConv's scalar nets excepted)."""
    out = _copy(sd)
    for bn in relu_bn_names(sd, family):
        if not _gates_everything(bn):
            out[bn + ".bias"] = (out[bn + ".bias"] - np.float32(shift)).astype(np.float32)
    return _sync_aliases(out)


VARIANCE_RANGE = (0.25, 4.0)       # 1 / sqrt(var) in [0.5, 2]: test_weight_variants_cpu.py holds the float64 logits below 1e4


def variance_spread(sd, lo=VARIANCE_RANGE[0], hi=VARIANCE_RANGE[1], seed=0):
    """running_var log-uniform in [lo, hi], every BatchNorm."""
    out = _copy(sd)
    for i, bn in enumerate(bn_names(sd)):
        rng = np.random.default_rng([seed, i])
        c = out[bn + ".running_var"].shape[0]
        out[bn + ".running_var"] = np.exp(rng.uniform(np.log(lo), np.log(hi), size=c)).astype(np.float32)
    return _sync_aliases(out)


def base_state_dict(family, seed=0):
    from interpret_quality_amd import synth
    return {"pointnet": synth.pointnet_state_dict, "pointnet2": synth.pointnet2_state_dict, "pointconv": synth.pointconv_state_dict,
            "dgcnn": synth.dgcnn_state_dict, "gcnn": synth.dgcnn_state_dict}[family](seed)


RESCALED_BNS = {"pointnet": 14, "pointnet2": 23, "pointconv": 32, "gcnn": 7, "dgcnn": 3}
# about half a standard deviation of a pre-activation (gamma ~ 1); PointNet++ and PointConv stack nine to twelve shifted layers and
# are a constant network from 0.5 on (float64 oracle: every logit the same for every cloud), so they get 0.3
NEGATIVE_SHIFT = {"pointnet": 0.5, "pointnet2": 0.3, "pointconv": 0.3, "gcnn": 0.5, "dgcnn": 0.5}


def variant(family, name):
    """The named variants the GPU tests build models from -> numpy state dict."""
    if name == "base":
        return base_state_dict(family, 0)
    if name in ("seed1", "seed2"):
        return base_state_dict(family, int(name[-1]))
    if name == "dead":
        return dead_channels(base_state_dict(family, 0), seed=3)[0]
    if name == "negshift":
        return negative_shift(base_state_dict(family, 0), family, NEGATIVE_SHIFT[family])
    if name == "varspread":
        return variance_spread(base_state_dict(family, 0), seed=4)
    if name == "rescaled12":
        return rescaled(base_state_dict(family, 0), family, 12, 5)[0]
    if name == "rescaled6":
        return rescaled(base_state_dict(family, 0), family, 6, 6)[0]
    raise ValueError(name)


# ---- the CPU oracle on a numpy state dict, in float32 or float64 ---------------------------------------------------------------

def oracle_forward(family, sd, clouds_bn3, dtype="float32", return_aux=False):
    """The CPU oracle of ``family`` on (B,N,3) clouds with the numpy state dict ``sd``, everything cast to ``dtype``.
    -> pointnet: (logits, trans_feat, crt[, aux]); the others: logits or (logits, aux).  Torch tensors."""
    import torch
    from oracle import ref_cpu as O
    dt = getattr(torch, dtype)
    tsd = {k: torch.from_numpy(np.asarray(v)).to(dt) for k, v in sd.items() if np.asarray(v).dtype.kind == "f"}
    x = torch.as_tensor(np.asarray(clouds_bn3)).to(dt).permute(0, 2, 1).contiguous()
    with torch.no_grad():
        if family == "pointnet":
            return O.pointnet_forward(tsd, x, return_aux=return_aux)
        if family == "pointnet2":
            return O.pointnet2_forward(tsd, x, return_aux=return_aux)
        if family == "pointconv":
            return O.pointconv_forward(tsd, x, return_aux=return_aux)
        return O.dgcnn_forward(tsd, x, 20, family == "gcnn", return_aux=return_aux)


def pooled_channels(family, aux):
    """The pooled layers of an oracle run as a list of (name, (rows, channels) float64 array): what a dead or all-negative channel
    shows up in.  PointNet: the trunk's pre-pool activations and the STNs' pooled layers; PointNet++ / PointConv: the stage
    outputs; DGCNN / GCNN: the EdgeConv outputs (LeakyReLU: a dead channel is its bias or 0.2 x it)."""
    def rows(t):            # (B,C,S) -> (B*S, C)
        return t.permute(0, 2, 1).reshape(-1, t.shape[1]).double().numpy()
    if family == "pointnet":
        return [("trunk", rows(aux["trunk"])), ("stn_pool", aux["stn_pool"].double().numpy()), ("fstn_pool", aux["fstn_pool"].double().numpy())]
    if family in ("pointnet2", "pointconv"):
        return [(k, rows(aux[k])) for k in ("l1_points", "l2_points")]
    return [(k, rows(aux[k])) for k in ("x1", "x2", "x3", "x4")]
