"""GPU: layer 1 of the PointNet chain kernel's bf16x3 instantiations on v_mfma_f32_16x16x32_bf16 (csrc/iq_pointnet_chain.h: l1_bf3,
stage0b_planes; every pn_chain_kernel<*, 3, *>).  One 200-point cloud, five regions (tests/chain_l1_cases.py).

(a) Wide-range layer-1 weights, seeds chain_l1_cases.SEEDS (0, 1, 2: every seed tried was kept): feat.fstn.conv1 with per-entry
    magnitudes log-uniform in 2^-10 .. 2^10 and mixed signs, fstn.fc3 scaled so that the regressed 64 x 64 transform (the trunk's
    layer-1 weights) spans 1e-8 .. 1e2 with cancelling pairs in every column.  Logits and feature transforms against the float64
    CPU oracle with the project's bar e(HIP) <= min(4 e(float32 oracle) + 1e-7, 1e-4), e(x) = max |x - float64| / max |float64|,
    and against the fp32-MFMA twin ("chain_l3_fp32") within 2e-6 of the largest logit.
(b) Row counts on both sides of every 16-row m-tile edge of layer 1: 1, 15, 16, 17, 32, 33, 64, 65, 80, 81, 96, 97, 192 and 193 rows
    (two labellings share them: no five region sizes give all fourteen) and the centre alone (the 1-row case); per count the
    product kernels, the 64-row twin ("chain_l3_single"), the dense forward on the materialised cloud and the coalition alone in a launch
    agree bit for bit on logits, feature transforms and arg-max rows.
(c) A row's result does not depend on its place: the same coalition through two labellings that order its rows differently gives
    the same pooled features, seen through the logits, the feature transform and the arg-max POINTS (every channel's maximum is
    attained by the same point; an exact tie between two points could differ and is not expected in 1024 channels of this cloud)."""
import numpy as np
import pytest
import torch

import chain_l1_cases as C
import weight_variants as V
from interpret_quality_amd import hip_ops, synth
from interpret_quality_amd.pointnet import PointNetCls
from interpret_quality_amd.tuning import tuned
from probes import rel_err

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def build_model(sd):
    m = PointNetCls(None)
    m.load_state_dict(synth.to_torch(sd))
    return m.to(dev()).eval()


@pytest.fixture(scope="module")
def cloud():
    data = torch.from_numpy(synth.make_cloud(61, 200)[0]).unsqueeze(0).to(dev())
    return {"data": data, "center": torch.mean(data, dim=1).contiguous()}


def run(model, cloud, rid, keep, **kw):
    d = dev()
    rid_t = torch.from_numpy(rid).to(d).reshape(1, -1)
    return model.engine().coalition_logits(cloud["data"], cloud["center"], rid_t, hip_ops.masks_to_tensor(list(keep), d), None,
                                           num_regions=int(rid.max()) + 1, return_trans_feat=True, **kw)


def dense(model, cloud, rid, keep):
    d = dev()
    rid_t = torch.from_numpy(rid).to(d)
    masked = hip_ops.mask_coalitions(cloud["data"][0].contiguous(), rid_t.contiguous(), hip_ops.masks_to_tensor(list(keep), d),
                                     cloud["center"].reshape(3).contiguous(), channel_first=True)
    return model(masked)                                                  # logits, (B,64,64) feature transforms, arg-max rows


# ---- (a) wide-range layer-1 weights -----------------------------------------------------------------------------------------------

def assert_within_the_oracles_error(name, got, ref32, ref64):
    e_hip, e_ref = rel_err(got, ref64), rel_err(ref32, ref64)
    bar = min(4 * e_ref + 1e-7, 1e-4)
    print("%-40s e_hip %.3g  e_ref %.3g  (bar %.3g)" % (name, e_hip, e_ref, bar))
    assert np.isfinite(got).all(), name
    assert e_hip <= bar, "%s: e_hip %.3g above min(4 x %.3g + 1e-7, 1e-4)" % (name, e_hip, e_ref)


@pytest.mark.parametrize("seed", C.SEEDS)
def test_wide_range_layer1_weights_against_float64_and_the_fp32_twin(cloud, seed):
    sd = C.wide_range_state_dict(seed)
    w = np.abs(sd["feat.fstn.conv1.weight"])
    assert w.min() < 2.0 ** -9 and w.max() > 2.0 ** 9 and (sd["feat.fstn.conv1.weight"] < 0).any()
    rid = C.labelling(C.SIZES_A, 5)
    keep = sorted(set(C.masks_for(C.SIZES_A, C.WANT_ROWS).values())) + [31]
    clouds = C.masked_clouds(cloud["data"][0].cpu().numpy(), cloud["center"].cpu().numpy(), rid, keep)
    o32 = V.oracle_forward("pointnet", sd, clouds, "float32")
    o64 = V.oracle_forward("pointnet", sd, clouds, "float64")
    l32, t32, l64, t64 = o32[0].numpy(), o32[1].numpy(), o64[0].numpy(), o64[1].numpy()
    assert np.isfinite(l32).all() and np.isfinite(t32).all() and np.abs(l32).max() < C.LOGIT_CAP       # the seed is a kept one
    assert np.abs(t64).max() / np.abs(t64).min() > 2.0 ** 20                                         # the transform's range

    model = build_model(sd)
    logits, tfp = run(model, cloud, rid, keep)
    tf = tfp.index_select(1, model.engine().weights.unpack_index).reshape(-1, 64, 64).cpu().numpy()
    tag = "seed %d " % seed
    assert_within_the_oracles_error(tag + "coalition logits", logits.cpu().numpy(), l32, l64)
    assert_within_the_oracles_error(tag + "coalition trans_feat", tf, t32, t64)
    d_logits, d_tf, _ = dense(model, cloud, rid, keep)
    assert_within_the_oracles_error(tag + "dense logits", d_logits.cpu().numpy(), l32, l64)
    assert_within_the_oracles_error(tag + "dense trans_feat", d_tf.cpu().numpy(), t32, t64)

    f32, tfp_f32 = tuned("chain_l3_fp32", lambda: run(model, cloud, rid, keep))
    err = (logits - f32).abs().max().item() / f32.abs().max().item()
    err_tf = (tfp - tfp_f32).abs().max().item() / tfp_f32.abs().max().item()
    print("%sagainst the fp32 twin: logits %.3g, feature transforms %.3g of the largest value" % (tag, err, err_tf))
    assert not torch.equal(logits, f32)                                   # two different kernels did run
    assert err < 2e-6 and err_tf < 2e-6


# ---- (b) row counts across every layer-1 tile edge --------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def model(pointnet_sd):
    m = PointNetCls(None)
    m.load_state_dict(pointnet_sd)
    return m.to(dev()).eval()


@pytest.mark.parametrize("sizes,seed", [(C.SIZES_A, 5), (C.SIZES_B, 6)])
def test_row_counts_across_the_tile_edges_bit_for_bit(model, cloud, sizes, seed):
    rid = C.labelling(sizes, seed)
    masks = C.masks_for(sizes, C.WANT_ROWS)
    keep = list(masks.values())
    got = run(model, cloud, rid, keep, return_crt=True)                     # logits, packed feature transforms, arg-max rows
    twin = tuned("chain_l3_single", lambda: run(model, cloud, rid, keep, return_crt=True))
    d_logits, d_tf, d_crt = dense(model, cloud, rid, keep)
    tf = got[1].index_select(1, model.engine().weights.unpack_index).reshape(-1, 64, 64)
    kept = np.stack([((k >> rid) & 1).astype(bool) for k in keep])
    for i, (rows, k) in enumerate(masks.items()):
        what = "%d rows (keep mask %d)" % (rows, k)
        assert int(kept[i].sum()) + (not kept[i].all()) == rows
        for a, b in zip(got, twin):
            assert torch.equal(a[i], b[i]), what + ": product against the 64-row twin"
        assert torch.equal(got[0][i], d_logits[i]) and torch.equal(tf[i], d_tf[i]), what + ": dense forward"
        # arg-max rows: the coalition path names points (200 = the centre), the dense forward rows of the materialised cloud, where
        # a masked row holds the centre: equal wherever the winner is a kept point, a masked row wherever it is the centre
        c, dc = got[2][i].cpu().numpy().astype(np.int64), d_crt[i].cpu().numpy().astype(np.int64)
        centre = c == 200
        assert (c[~centre] == dc[~centre]).all() and kept[i][c[~centre]].all() and not kept[i][dc[centre]].any(), what + ": arg-max rows"
        alone = run(model, cloud, rid, [k], return_crt=True)
        for a, b in zip(got, alone):
            assert torch.equal(a[i], b[0]), what + ": the coalition alone in a launch"
    assert sorted(set(C.masks_for(C.SIZES_A, C.WANT_ROWS)) | set(C.masks_for(C.SIZES_B, C.WANT_ROWS))) == list(C.WANT_ROWS)


# ---- (c) a row's result does not depend on its place -------------------------------------------------------------------------------

@pytest.mark.parametrize("npts", (40, 100, 150))
def test_a_rows_result_does_not_depend_on_its_place(model, cloud, npts):
    """The same ``npts`` points as regions {0, 1} of two labellings: the first lists them in point order split at one third, the
    second deals them to the two regions at random, so a point sits in another 16-row m-tile, lane group and (150 rows) chunk."""
    rng = np.random.default_rng(npts)
    members = np.sort(rng.permutation(200)[:npts])
    rest = np.setdiff1d(np.arange(200), members)
    rid_a, rid_b = np.empty(200, np.int32), np.empty(200, np.int32)
    rid_a[rest] = rid_b[rest] = 2 + rng.integers(0, 3, size=rest.size)
    rid_a[members] = (np.arange(npts) >= npts // 3).astype(np.int32)
    rid_b[members] = rng.integers(0, 2, size=npts)
    order = lambda rid: np.concatenate([np.flatnonzero(rid == 0), np.flatnonzero(rid == 1)])
    assert not np.array_equal(order(rid_a), order(rid_b)) and sorted(order(rid_b)) == sorted(order(rid_a))
    a = run(model, cloud, rid_a, [3], return_crt=True)
    b = run(model, cloud, rid_b, [3], return_crt=True)
    assert torch.equal(a[0], b[0]), "logits"
    assert torch.equal(a[1], b[1]), "feature transforms"
    assert torch.equal(a[2], b[2]), "arg-max points"
