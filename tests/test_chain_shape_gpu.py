"""GPU: layer 3 of the PointNet chain kernel on v_mfma_f32_16x16x32_bf16 (csrc/iq_pointnet_chain.h, l3_pass_bf3 / l3_pass_bf3_2x2).

The m-tiles are 16 rows now and a column's rows are spread over four lane groups, so the cases are coalitions whose row counts
cover every residue mod 16 and the chunk edges: 1, 15, 16, 17, 31, 32, 33, 63, 64, 65 rows (and 2 .. 14), and the full cloud
(1024 rows).  Bars (none of them new): the bf16x3 kernel against the fp32-MFMA twin ("chain_l3_fp32") within 2e-6 of the largest
value, on logits and feature transforms (tests/test_hip_parity.py's bar: the two differ only in the order of float32 additions);
two n-tiles per pass (default) against one ("chain_l3_single") bit for bit; a coalition alone in a launch against the same coalition inside a
batch bit for bit; the dense forward on the materialised cloud against the coalition path bit for bit, and its crt_points (the
arg-max variant of the kernel) consistent with the pooled maxima: the same critical POINTS as the coalition path's arg-max, the
lowest row among identical points (tie rule), and the same points after the rows are permuted (a row's result depends neither on
its tile nor on its lane group)."""
import numpy as np
import pytest
import torch

from interpret_quality_amd import hip_ops, synth, tuning
from interpret_quality_amd.pointnet import PointNetCls

pytestmark = pytest.mark.gpu

EDGE_ROWS = [15, 16, 17, 31, 32, 33, 63, 64, 65] + list(range(2, 15))      # rows = region size + the centre


@pytest.fixture(scope="module")
def model(pointnet_sd):
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    m = PointNetCls(None)
    m.load_state_dict(pointnet_sd)
    return m.to(torch.device("cuda:0")).eval()


@pytest.fixture(scope="module")
def case():
    """One cloud of 1024 points, region r < 22 of EDGE_ROWS[r] - 1 points, region 22 the rest; keep masks: nothing (the centre
    alone: 1 row), every single edge region, everything (1024 rows, no centre), and pairs / triples of regions."""
    d = torch.device("cuda:0")
    rng = np.random.default_rng(16)
    pts, _ = synth.make_cloud(7)
    sizes = [r - 1 for r in EDGE_ROWS]
    sizes.append(1024 - sum(sizes))
    rid = np.repeat(np.arange(len(sizes)), sizes).astype(np.int32)
    rng.shuffle(rid)
    nreg = len(sizes)
    keep = [0] + [1 << r for r in range(nreg - 1)] + [(1 << nreg) - 1]
    keep += [(1 << 0) | (1 << 3), (1 << 2) | (1 << 5) | (1 << 9), (1 << 6) | (1 << 7), (1 << 8) | (1 << 22), (1 << 22)]
    rows = np.array([int(np.isin(rid, [r for r in range(nreg) if (k >> r) & 1]).sum()) for k in keep])
    rows = rows + (rows < 1024)
    assert set(rows.tolist()) >= set([1, 1024] + EDGE_ROWS) and len(set((rows % 16).tolist())) == 16
    data = torch.from_numpy(pts).unsqueeze(0).to(d)
    return {"data": data, "center": torch.mean(data, dim=1).contiguous(), "rid": torch.from_numpy(rid).to(d).reshape(1, -1),
            "keep": keep, "keep_t": hip_ops.masks_to_tensor(keep, d), "nreg": nreg, "rows": rows}


def test_every_row_residue_against_the_fp32_twin_and_the_single_tile_pass(model, case):
    eng = model.engine()
    run = lambda: eng.coalition_logits(case["data"], case["center"], case["rid"], case["keep_t"], None, num_regions=case["nreg"],
                                       return_trans_feat=True)
    got, tf = run()
    f32, tf_f32 = tuning.tuned("chain_l3_fp32", run)
    one, tf_one = tuning.tuned("chain_l3_single", run)
    assert torch.isfinite(got).all() and torch.isfinite(tf).all()
    err = (got - f32).abs().max().item() / f32.abs().max().item()
    err_tf = (tf - tf_f32).abs().max().item() / tf_f32.abs().max().item()
    print("bf16x3 against the fp32 twin: logits %.3g, feature transforms %.3g of the largest value" % (err, err_tf))
    assert not torch.equal(got, f32)                                  # two different kernels did run
    assert err < 2e-6 and err_tf < 2e-6
    assert torch.equal(got, one) and torch.equal(tf, tf_one)


def test_a_coalition_alone_equals_the_same_coalition_in_a_batch(model, case):
    eng = model.engine()
    d = case["data"].device
    got = eng.coalition_logits(case["data"], case["center"], case["rid"], case["keep_t"], None, num_regions=case["nreg"])
    for i, k in enumerate(case["keep"]):
        alone = eng.coalition_logits(case["data"], case["center"], case["rid"], hip_ops.masks_to_tensor([k], d), None,
                                     num_regions=case["nreg"])
        assert torch.equal(alone[0], got[i]), "coalition %d (%d rows)" % (i, case["rows"][i])


def test_dense_forward_and_its_arg_max_rows_agree_with_the_coalition_path(model, case):
    eng = model.engine()
    data, center, rid, keep_t = case["data"], case["center"], case["rid"], case["keep_t"]
    got, crt_c = eng.coalition_logits(data, center, rid, keep_t, None, num_regions=case["nreg"], return_crt=True)
    dense = hip_ops.mask_coalitions(data[0].contiguous(), rid[0].contiguous(), keep_t, center.reshape(3).contiguous(), channel_first=True)
    logits, _, crt = model(dense)                                       # (B,3,1024) materialised clouds
    assert torch.equal(logits, got)
    pts = dense.permute(0, 2, 1).cpu().numpy()                           # (B,1024,3)
    crt = crt.cpu().numpy()
    src = np.concatenate([data[0].cpu().numpy(), center.cpu().numpy().reshape(1, 3)])     # index 1024 = the centre
    crt_c = crt_c.cpu().numpy()
    for b in range(pts.shape[0]):
        assert crt[b].min() >= 0 and crt[b].max() < 1024
        crit = pts[b][crt[b]]                                            # (1024,3) the critical point of every channel
        # the same critical points as the coalition path's own arg-max (there: index into the source cloud, 1024 = the centre)
        assert np.array_equal(crit, src[crt_c[b]]), "coalition %d (%d rows)" % (b, case["rows"][b])
        # tie rule: among identical points (every masked point is the centre) the lowest row
        first = np.array([np.flatnonzero((pts[b] == p).all(axis=1))[0] for p in crit])
        assert np.array_equal(first, crt[b]), "coalition %d (%d rows)" % (b, case["rows"][b])
    # rows permuted: the same pooled maxima (bitwise logits) attained by the same points
    perm = torch.from_numpy(np.random.default_rng(5).permutation(1024)).to(dense.device)
    logits_p, _, crt_p = model(dense[:, :, perm].contiguous())
    assert torch.equal(logits_p, logits)
    pts_p = pts[:, perm.cpu().numpy(), :]
    crt_p = crt_p.cpu().numpy()
    for b in range(pts.shape[0]):
        assert np.array_equal(pts_p[b][crt_p[b]], pts[b][crt[b]]), "coalition %d (%d rows)" % (b, case["rows"][b])
