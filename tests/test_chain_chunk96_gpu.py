"""GPU: the 96-row chunks of the PointNet chain kernel's product instantiations (csrc/iq_pointnet_chain.h, chain_bf3_96:
pn_chain_kernel<kFstn | kTrunk, 3, false>; the 64-row twins are the modes kFstn64 / kTrunk64).

The cases are coalitions whose row counts sit on every edge of the 32-row m-tiles and of the 96-row chunks: 1, 31, 32, 33, 63, 64,
65, 95, 96, 97, 127, 128, 129, 159, 160, 161, 191, 192, 193 rows and the full cloud (1024 rows: ten full chunks and a 64-row
remainder).  Bars (tests/test_chain_shape_gpu.py's, none of them new): the 64-row kernel with one n-tile per pass ("chain_l3_single")
bit for bit, on logits and feature transforms; the fp32-MFMA twin ("chain_l3_fp32") within 2e-6 of the largest value; a coalition alone in
a launch against the same coalition inside the batch bit for bit; the dense forward on the materialised cloud (the 64-row arg-max
kernel) bit for bit.

The 96-row kernel's fetch lanes read whole 96-row chunks of a row list, so the lists are padded to the 96-rounding of the row
count where that ends later than the 64-rounding.  Three cases read that padding, each bit for bit against the dense forward:
N = 100 with 4 regions and every keep mask (65 .. 100 rows: 96-rounding 96 or 192, 64-rounding 128), N = 200 as a wide game of
128 regions, and one dense coalition of N = 4096 (43 chunks: the last one ends at list entry 4127)."""
import numpy as np
import pytest
import torch

from interpret_quality_amd import hip_ops, synth, tuning
from interpret_quality_amd.pointnet import PointNetCls

pytestmark = pytest.mark.gpu

ROWS = [1, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 159, 160, 161, 191, 192, 193, 1024]


@pytest.fixture(scope="module")
def model(pointnet_sd):
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    m = PointNetCls(None)
    m.load_state_dict(pointnet_sd)
    return m.to(torch.device("cuda:0")).eval()


@pytest.fixture(scope="module")
def case():
    """One cloud of 1024 points; the kept-point counts ROWS[i] - 1 (the centre is the last row) are nested: region r holds the
    difference between two consecutive counts, coalition i keeps the first i regions; the last coalition keeps everything
    (1024 rows, no centre)."""
    d = torch.device("cuda:0")
    pts, _ = synth.make_cloud(11)
    kept = [r - 1 for r in ROWS[:-1]]                       # 0, 30, 31, 32, 62, ...
    sizes = [b - a for a, b in zip(kept[:-1], kept[1:])]
    sizes.append(1024 - sum(sizes))
    nreg = len(sizes)
    rid = np.repeat(np.arange(nreg), sizes).astype(np.int32)
    np.random.default_rng(96).shuffle(rid)
    keep = [(1 << i) - 1 for i in range(nreg)] + [(1 << nreg) - 1]
    rows = np.array([int(np.isin(rid, [r for r in range(nreg) if (k >> r) & 1]).sum()) for k in keep])
    rows = rows + (rows < 1024)
    assert rows.tolist() == ROWS
    data = torch.from_numpy(pts).unsqueeze(0).to(d)
    return {"data": data, "center": torch.mean(data, dim=1).contiguous(), "rid": torch.from_numpy(rid).to(d).reshape(1, -1),
            "keep": keep, "keep_t": hip_ops.masks_to_tensor(keep, d), "nreg": nreg, "rows": rows}


@pytest.fixture(scope="module")
def batch(model, case):
    """logits and feature transforms of the batch from the product kernels: computed once, read by every test"""
    return model.engine().coalition_logits(case["data"], case["center"], case["rid"], case["keep_t"], None,
                                           num_regions=case["nreg"], return_trans_feat=True)


def test_chunk_edges_against_the_64_row_kernel_and_the_fp32_twin(model, case, batch):
    eng = model.engine()
    run = lambda: eng.coalition_logits(case["data"], case["center"], case["rid"], case["keep_t"], None, num_regions=case["nreg"],
                                       return_trans_feat=True)
    got, tf = batch
    f32, tf_f32 = tuning.tuned("chain_l3_fp32", run)
    one, tf_one = tuning.tuned("chain_l3_single", run)
    assert torch.isfinite(got).all() and torch.isfinite(tf).all()
    err = (got - f32).abs().max().item() / f32.abs().max().item()
    err_tf = (tf - tf_f32).abs().max().item() / tf_f32.abs().max().item()
    print("96-row bf16x3 against the fp32 twin: logits %.3g, feature transforms %.3g of the largest value" % (err, err_tf))
    assert not torch.equal(got, f32)                                  # two different kernels did run
    assert err < 2e-6 and err_tf < 2e-6
    for i, r in enumerate(case["rows"]):
        assert torch.equal(got[i], one[i]) and torch.equal(tf[i], tf_one[i]), "coalition %d (%d rows)" % (i, r)


def test_a_coalition_alone_equals_the_same_coalition_in_the_batch(model, case, batch):
    eng = model.engine()
    d = case["data"].device
    got, tf = batch
    for i, k in enumerate(case["keep"]):
        alone, tf_alone = eng.coalition_logits(case["data"], case["center"], case["rid"], hip_ops.masks_to_tensor([k], d), None,
                                               num_regions=case["nreg"], return_trans_feat=True)
        assert torch.equal(alone[0], got[i]) and torch.equal(tf_alone[0], tf[i]), "coalition %d (%d rows)" % (i, case["rows"][i])


def test_dense_forward_equals_the_coalition_path(model, case, batch):
    dense = hip_ops.mask_coalitions(case["data"][0].contiguous(), case["rid"][0].contiguous(), case["keep_t"],
                                    case["center"].reshape(3).contiguous(), channel_first=True)
    logits = model(dense)[0]                                            # (B,3,1024) materialised clouds, 64-row arg-max kernel
    for i, r in enumerate(case["rows"]):
        assert torch.equal(logits[i], batch[0][i]), "coalition %d (%d rows)" % (i, r)


def test_argmax_trunks_equal_their_plain_twins_and_name_kept_points(model, case, batch):
    """The arg-max trunks against the trunks without arg-max, logits bit for bit: pn_chain_kernel<kTrunk, 2, true> against
    <kTrunk, 2, false> with its 16-row tails (twin "chain_l3_fp32", documented bit-identical), and in the product path
    <kTrunk, 3, true> (64-row chunks) against <kTrunk, 3, false> (96-row chunks).  Every arg-max index is a kept point of its
    coalition, or N (the centre) in a coalition that has a centre row; the coalition of the centre alone names nothing else."""
    eng = model.engine()
    run = lambda **kw: eng.coalition_logits(case["data"], case["center"], case["rid"], case["keep_t"], None, num_regions=case["nreg"], **kw)
    with tuning.twin("chain_l3_fp32"):
        f32 = run()
        f32_arg, crt_f32 = run(return_crt=True)
    bf3_arg, crt_bf3 = run(return_crt=True)
    assert torch.equal(f32_arg, f32)
    assert torch.equal(bf3_arg, batch[0])
    assert not torch.equal(f32, batch[0])                             # two different pairs of kernels did run
    n, rid = case["data"].shape[1], case["rid"][0].long()
    for name, crt in (("fp32", crt_f32), ("bf16x3", crt_bf3)):
        for i, k in enumerate(case["keep"]):
            in_k = torch.tensor([(k >> r) & 1 for r in range(case["nreg"])], dtype=torch.bool, device=rid.device)
            allowed = torch.cat([in_k[rid], torch.tensor([bool(case["rows"][i] < n)], device=rid.device)])   # entry N: the centre row
            idx = crt[i].long()
            assert ((idx >= 0) & (idx <= n)).all(), "%s, coalition %d (%d rows)" % (name, i, case["rows"][i])
            assert allowed[idx].all(), "%s, coalition %d (%d rows)" % (name, i, case["rows"][i])
        assert (crt[0] == n).all(), name                              # coalition 0 keeps nothing: the centre alone


def _cloud(seed, n):
    d = torch.device("cuda:0")
    data = torch.from_numpy(synth.make_cloud(seed, n)[0]).unsqueeze(0).to(d)
    return data, torch.mean(data, dim=1).contiguous()


def test_row_list_padding_100_points_every_mask(model):
    """35 + 30 + 20 + 15 points: every coalition of 65 .. 99 rows has its last 96-row chunk end at entry 95 or 191 of a list
    that the 64-rounding would have padded to 128 only."""
    data, center = _cloud(21, 100)
    rid = np.repeat(np.arange(4), [35, 30, 20, 15]).astype(np.int32)
    np.random.default_rng(100).shuffle(rid)
    rid_t = torch.from_numpy(rid).to(data.device).reshape(1, -1)
    keep_t = hip_ops.masks_to_tensor(list(range(16)), data.device)
    got = model.engine().coalition_logits(data, center, rid_t, keep_t, None, num_regions=4)
    dense = hip_ops.mask_coalitions(data[0].contiguous(), rid_t[0].contiguous(), keep_t, center.reshape(3).contiguous(), channel_first=True)
    want = model(dense)[0]
    for k in range(16):
        assert torch.equal(got[k], want[k]), "keep mask %d" % k


def test_row_list_padding_200_points_wide_game(model):
    """R = 128 (two keep words, so no narrow twin): the row lists come from pn_rows_wide_kernel; 66, 102, 130, 162, 200 and 1 rows"""
    data, center = _cloud(22, 200)
    r = 128
    rid = np.concatenate([np.arange(r), np.random.default_rng(200).integers(0, r, 200 - r)]).astype(np.int32)
    np.random.default_rng(201).shuffle(rid)
    order = np.argsort(np.bincount(rid, minlength=r), kind="stable")     # regions, fewest points first
    member = np.zeros((6, r), dtype=bool)
    for i, want_pts in enumerate([65, 100, 129, 160]):
        acc = 0
        for reg in order:                                             # add regions until the coalition holds at least want_pts points
            if acc >= want_pts:
                break
            member[i, reg] = True
            acc += int((rid == reg).sum())
    member[4, :] = True                                               # everything: 200 rows, no centre
    keep = np.stack([hip_ops.region_words(np.flatnonzero(m), r) for m in member])          # row 5: nothing kept, the centre alone
    kept = member[:, rid].sum(axis=1)
    rows = (kept + (kept < 200)).tolist()                             # the centre joins wherever a point is masked
    assert rows == [66, 102, 130, 162, 200, 1], rows
    # 102, 200 and 1 rows: the 96-rounding ends past the 64-rounding, so the last chunk reads padding that only
    # pn_rows_wide_kernel's wider rule writes
    assert sum(-(-n // 96) * 96 > -(-n // 64) * 64 for n in rows) >= 3, rows
    kw = hip_ops.wide_masks_to_tensor(keep, data.device)
    rid_t = torch.from_numpy(rid).to(data.device).reshape(1, -1)
    got = model.coalition_logits_wide(data, center, rid_t, kw, None, num_regions=r)
    masked = hip_ops.mask_coalitions_wide(data[0].contiguous(), rid_t[0].contiguous(), kw, center[0].contiguous(), r, channel_first=True)
    want = model(masked)[0]
    for i in range(6):
        assert torch.equal(got[i], want[i]), "coalition %d (%d rows)" % (i, rows[i])


def test_row_list_padding_one_dense_coalition_of_4096_points(model):
    """4096 rows = 42 full chunks and 64 rows: the fetch lanes of the last chunk read list entries 4032 .. 4127 (stride 4160)"""
    data, center = _cloud(23, 4096)
    rid = torch.from_numpy((np.arange(4096) % 2).astype(np.int32)).to(data.device).reshape(1, -1)
    got = model.engine().coalition_logits(data, center, rid, hip_ops.masks_to_tensor([3], data.device), None, num_regions=2)
    want = model(data.permute(0, 2, 1).contiguous())[0]
    assert torch.equal(got, want)
