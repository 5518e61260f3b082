"""GPU: PointNet's fstn.fc3 (256 -> 4096) on the bf16 matrix pipe.  iq_pointnet_coalitions splits the layer's float32 image into
three bf16 terms on the device, per call (the weight descriptor carries no bf16x3 image of it), and the layer then runs like
the other wide heads.  64 points in 4 regions, 1, 5 and 130 coalitions (one row tile of the layer, and two with a partial one):
(a) coalition path = dense forward on the materialised clouds = the coalition alone, bit for bit (logits, feature transforms);
(b) under the twin "dense_fp32" (dense layers on the fp32 MFMA: no split) the feature transforms are NOT the same bits;
(c) against a float64 run of the CPU oracle the bar of tests/test_stress_weights_gpu.py,
    e(HIP) <= min(4 e(float32 oracle) + 1e-7, 1e-4), for the base weights and the variance-spread variant;
and without a feature STN (feature_transform=False) the trunk still gets the packed identity, exactly."""
import argparse

import numpy as np
import pytest
import torch

import probes
import weight_variants as V
from interpret_quality_amd import hip_ops, synth
from interpret_quality_amd.pointnet import PointNetCls
from interpret_quality_amd.tuning import tuned
from probes import rel_err

pytestmark = pytest.mark.gpu

N, R = 64, 4
BATCHES = (1, 5, 130)


def dev():
    return torch.device("cuda:0")


_CASE = {}


def case():
    """The cloud, its regions and 130 coalitions (every one of the 16 masks occurs; the first five: empty, full, three others),
    materialised once."""
    if not _CASE:
        d = dev()
        rng = np.random.default_rng(64)
        rid = np.repeat(np.arange(R), N // R).astype(np.int32)
        rng.shuffle(rid)
        keep = [0, 15, 5, 8, 14] + list(range(16)) + [int(k) for k in rng.integers(0, 16, size=130 - 21)]
        data = torch.from_numpy(synth.make_cloud(43, N)[0]).unsqueeze(0).to(d)
        center = torch.mean(data, dim=1).contiguous()
        rid_t = torch.from_numpy(rid).to(d).reshape(1, -1)
        keep_t = hip_ops.masks_to_tensor(keep, d)
        masked = hip_ops.mask_coalitions(data[0].contiguous(), rid_t[0].contiguous(), keep_t, center.reshape(3).contiguous())
        _CASE.update(data=data, center=center, rid=rid_t, keep=keep, keep_t=keep_t, masked=masked, masked_h=masked.cpu().numpy())
    return _CASE


def run(eng, keep_t):
    c = case()
    return eng.coalition_logits(c["data"], c["center"], c["rid"], keep_t, None, num_regions=R, return_trans_feat=True)


def unpacked(eng, tfp):
    return tfp.index_select(1, eng.weights.unpack_index).reshape(-1, 64, 64)


@pytest.mark.parametrize("b", BATCHES)
def test_coalition_dense_and_alone_are_the_same_bits(b):
    model, _ = probes.coalition_model("pointnet", dev())
    eng, c = model.engine(), case()
    logits, tfp = run(eng, c["keep_t"][:b].contiguous())
    d_logits, d_tf, _ = model(c["masked"][:b].permute(0, 2, 1).contiguous())
    assert torch.equal(d_logits, logits) and torch.equal(d_tf, unpacked(eng, tfp))
    for i in sorted({0, b // 2, b - 1}):
        alone, tf_alone = run(eng, c["keep_t"][i:i + 1].contiguous())
        assert torch.equal(alone[0], logits[i]) and torch.equal(tf_alone[0], tfp[i]), "coalition %d of %d" % (i, b)
    # (b) the fp32-MFMA twin of the dense layers computes other bits: fc3 is on the bf16 pipe by default
    _, tfp_f32 = tuned("dense_fp32", lambda: run(eng, c["keep_t"][:b].contiguous()))
    assert not torch.equal(tfp_f32, tfp)
    assert (tfp_f32 - tfp).abs().max().item() < 1e-5 * tfp.abs().max().item()
    # and the 128-row launch of the heads the same ones
    l128, tfp128 = tuned("dense_tile128", lambda: run(eng, c["keep_t"][:b].contiguous()))
    assert torch.equal(l128, logits) and torch.equal(tfp128, tfp)


@pytest.mark.parametrize("variant", ("base", "varspread"))
def test_feature_transforms_against_float64(variant):
    """Observed e(HIP) / e(float32 oracle) on the feature transforms: printed; DESIGN.md 5a records the largest."""
    model, _ = probes.coalition_model("pointnet", dev(), variant)
    eng, c = model.engine(), case()
    sd = V.variant("pointnet", variant)
    ref = {dt: V.oracle_forward("pointnet", sd, c["masked_h"], dt) for dt in ("float32", "float64")}
    for b in BATCHES:
        logits, tfp = run(eng, c["keep_t"][:b].contiguous())
        for name, got, i in (("logits", logits.cpu().numpy(), 0), ("trans_feat", unpacked(eng, tfp).cpu().numpy(), 1)):
            r32, r64 = ref["float32"][i].numpy()[:b], ref["float64"][i].numpy()[:b]
            e_hip, e_ref = rel_err(got, r64), rel_err(r32, r64)
            bar = min(4 * e_ref + 1e-7, 1e-4)
            print("%s B=%d %-10s e_hip %.3g  e_ref %.3g  e_hip / e_ref %.2f  (bar %.3g)" % (variant, b, name, e_hip, e_ref, e_hip / max(e_ref, 1e-30), bar))
            assert np.isfinite(got).all() and e_hip <= bar, (variant, b, name, e_hip, e_ref)


def test_without_a_feature_stn_the_trunk_still_gets_the_packed_identity():
    m = PointNetCls(argparse.Namespace(dataset="modelnet10", feature_transform=False))
    m.load_state_dict(synth.to_torch(synth.pointnet_state_dict(0, feature_transform=False)))
    m = m.to(dev()).eval()
    eng, c = m.engine(), case()
    logits, tfp = run(eng, c["keep_t"])
    eye = torch.eye(64, device=dev()).expand(len(c["keep"]), 64, 64)
    assert torch.equal(unpacked(eng, tfp), eye)                                # the packed identity, every coalition
    d_logits, d_tf, _ = m(c["masked"].permute(0, 2, 1).contiguous())
    assert d_tf is None and torch.equal(d_logits, logits)
    for name in ("dense_fp32", "dense_tile128"):                               # no split and no fc3 launch either way
        _, tfp_t = tuned(name, lambda: run(eng, c["keep_t"]))
        assert torch.equal(tfp_t, tfp)
    l128, _ = tuned("dense_tile128", lambda: run(eng, c["keep_t"]))
    assert torch.equal(l128, logits)
