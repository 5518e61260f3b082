"""GPU parity: DGCNN / GCNN (kNN, EdgeConv, full models, interaction path) against golden vectors from
the reference.  kNN is index-valued with arbitrary tie order among exact duplicates, so neighbour SETS
are compared modulo distance ties."""
import argparse

import numpy as np
import pytest
import torch

from conftest import assert_close_elementwise, load_golden
from interpret_quality_amd import hip_ops, interaction, synth, tuning
from interpret_quality_amd.dgcnn import DGCNN_cls, GCNN_cls

pytestmark = pytest.mark.gpu
RTOL = 1e-4


def dev():
    return torch.device("cuda:0")


def rel_err(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


@pytest.fixture(scope="module")
def oracle():
    from oracle import ref_cpu
    return ref_cpu


@pytest.fixture(scope="module")
def clouds():
    g = load_golden("dgcnn.npz")
    pts, _ = synth.make_cloud(0)
    data = torch.from_numpy(pts).unsqueeze(0)
    center = torch.mean(data, dim=1).squeeze()
    half = data.clone()
    half[0, g["region_id"] >= 16, :] = center
    return torch.cat([data, half], dim=0)  # (2,1024,3): raw + half-masked


def make(cls):
    m = cls(argparse.Namespace(dataset="modelnet10", k=20))
    m.load_state_dict(synth.to_torch(synth.dgcnn_state_dict(0)))
    return m.to(dev()).eval()


def knn_set_mismatches(got, want, x_cf):
    """rows whose neighbour sets differ must differ only by candidates at (numerically) tied distance"""
    inner = torch.matmul(x_cf.transpose(2, 1), x_cf) * -2
    xx = torch.sum(x_cf ** 2, dim=1, keepdim=True)
    dist = (-xx - inner - xx.transpose(2, 1)).numpy()
    bad = 0
    for b in range(got.shape[0]):
        for i in range(got.shape[1]):
            sg, sw = set(got[b, i].tolist()), set(want[b, i].tolist())
            assert len(sg) == 20, "duplicate neighbour in row (%d,%d)" % (b, i)
            if sg != sw:
                dg = np.sort(dist[b, i, list(sg - sw)])
                dw = np.sort(dist[b, i, list(sw - sg)])
                scale = max(1.0, float(np.abs(dist[b, i]).max()))
                # float32 noise of the expanded form, plus the band inside which knn_refine_kernel ranks by exact distances
                # (csrc/iq_dgcnn_knn.h kNearTie: 1e-5 of 2 (|q|^2 + |q - k|^2))
                band = 2e-5 * (float(xx[b, 0, i]) + float(np.abs(dw).max()))
                assert np.allclose(dg, dw, rtol=0, atol=2e-6 * scale + band), (b, i, dg, dw)
                bad += 1
    return bad


def test_knn_xyz_and_feature_space(clouds, oracle):
    g = load_golden("dgcnn.npz")
    got = hip_ops.knn(clouds.to(dev()).contiguous(), 20).cpu().numpy()
    x_cf = clouds.permute(0, 2, 1).contiguous()
    nbad = knn_set_mismatches(got, g["knn_xyz"].astype(np.int32), x_cf)
    # feature space (C = 64): layer-1 output of the oracle as input
    sd = synth.to_torch(synth.dgcnn_state_dict(0))
    with torch.no_grad():
        _, aux = oracle.dgcnn_forward(sd, x_cf, 20, False, return_aux=True)
    x1 = aux["x1"]                                           # (2,64,1024)
    got64 = hip_ops.knn(x1.permute(0, 2, 1).contiguous().to(dev()), 20).cpu().numpy()
    nbad += knn_set_mismatches(got64, g["knn_feat64"].astype(np.int32), x1)
    # knn_set_mismatches already proved every difference is a tie; the half-masked cloud has 512 identical
    # rows (plus their neighbours) whose ties resolve arbitrarily, the raw cloud must match exactly
    assert nbad <= 2 * 640
    assert knn_set_mismatches(got[:1], g["knn_xyz"][:1].astype(np.int32), x_cf[:1]) == 0
    assert knn_set_mismatches(got64[:1], g["knn_feat64"][:1].astype(np.int32), x1[:1]) == 0


@pytest.mark.parametrize("arith", ["bf16x3", "fp32"])
@pytest.mark.parametrize("c", [64, 128])
def test_knn_near_ties_are_ranked_by_exact_distances(c, arith):
    """Feature-space graphs: where the float32 expanded form -|q|^2 + 2 q.k - |k|^2 cannot separate the 20th from the 21st
    nearest, knn_refine_kernel ranks by -sum (q - k)^2 in float64 (what the reference's float64 run sees).  Rows are planted
    with near-ties at the boundary (triplets of keys whose distances to a query differ by a few 1e-5 of the distance, below the float32 noise of the expanded form); the neighbour sets must
    equal the float64 top-20 of the SAME float32 features for every query whose exact 20th / 21st gap exceeds 1e-6 of the
    distance (a gap the float32 differences resolve), while the float32-only ranking (twin "knn_fp32_rank") provably gets some
    of them wrong - so the test has power."""
    rng = np.random.default_rng(c)
    b, n = 2, 512
    x = rng.standard_normal((b, n, c)).astype(np.float32) + 3.0   # large common offset: |x|^2 >> |x_i - x_j|^2, strong cancellation
    for k in range(0, n - 2, 3):    # triplets x[k], x[k] + tiny, x[k] + tiny': a query's ranks run self + 2 siblings, then whole
        for t in (1, 2):            # triplets (4-6, ..., 19-21) - the 20 | 21 boundary always falls INSIDE a triplet
            x[:, k + t] = x[:, k] + (rng.standard_normal((b, c)) * 2e-4).astype(np.float32)
    xt = torch.from_numpy(x).to(dev())
    x64 = x.astype(np.float64)
    exact = -((x64[:, :, None, :] - x64[:, None, :, :]) ** 2).sum(-1)            # (b,n,n)
    order = np.argsort(-exact, axis=-1, kind="stable")
    top = np.take_along_axis(exact, order[:, :, :21], axis=-1)
    decidable = (top[:, :, 19] - top[:, :, 20]) > 1e-6 * np.abs(top[:, :, 20])

    def wrong(got):
        n_bad = 0
        for bi in range(b):
            for i in range(n):
                if decidable[bi, i] and set(got[bi, i].tolist()) != set(order[bi, i, :20].tolist()):
                    n_bad += 1
        return n_bad

    # the inner products: fp32 MFMA | three-term bf16 products (the default)
    with tuning.twin("knn_fp32_mfma" if arith == "fp32" else None):
        got = hip_ops.knn(xt, 20).cpu().numpy()
    assert all(len(set(r.tolist())) == 20 for r in got.reshape(-1, 20))
    with tuning.twin("knn_fp32_rank"):
        got32 = hip_ops.knn(xt, 20).cpu().numpy()
    n_dec = int(decidable.sum())
    print("C=%d %s: %d of %d queries decidable; wrong neighbour sets: refined %d, float32 ranking only %d" % (c, arith, n_dec, b * n, wrong(got), wrong(got32)))
    assert n_dec > 0.9 * b * n
    assert wrong(got) == 0
    assert wrong(got32) > 0


@pytest.mark.parametrize("cls,name", [(DGCNN_cls, "dgcnn"), (GCNN_cls, "gcnn")])
def test_forward_matches_reference(clouds, cls, name):
    g = load_golden("dgcnn.npz")
    model = make(cls)
    logits = model(clouds.permute(0, 2, 1).contiguous().to(dev()))
    assert rel_err(logits.cpu().numpy(), g["raw_logits_" + name]) < RTOL
    assert_close_elementwise(logits.cpu().numpy(), g["raw_logits_" + name])   # and element-wise, with an absolute floor (conftest.py)


def knn_min_margin(p, c, g, tag):
    """Smallest relative gap between the 20th and 21st nearest candidates (exact ties excluded) over all
    rows and the three feature-space graphs of interaction cloud (pair p, row c), from the CPU oracle."""
    from oracle import ref_cpu as O
    pts, _ = synth.make_cloud(0)
    data = torch.from_numpy(pts).unsqueeze(0)
    center = torch.mean(data, dim=1).squeeze()
    ri, rj = g["pairs"][p]
    masked = O.interaction_masked_batch(data.permute(0, 2, 1), center, g["region_id"], ri, rj, g[tag + "_contexts"][p])
    x = masked[c:c + 1].contiguous()
    with torch.no_grad():
        _, aux = O.dgcnn_forward(synth.to_torch(synth.dgcnn_state_dict(0)), x, 20, False, return_aux=True)
        best = 1.0
        for t in (aux["x1"], aux["x2"], aux["x3"]):
            inner = torch.matmul(t.transpose(2, 1), t) * -2
            xx = torch.sum(t ** 2, dim=1, keepdim=True)
            d = (-xx - inner - xx.transpose(2, 1))[0]
            top = d.topk(40, dim=-1)[0]
            gap = (top[:, 19:20] - top[:, 20:])                     # 20th minus later candidates
            gap = torch.where(gap > 0, gap, torch.full_like(gap, float("inf"))).min(dim=1)[0]
            best = min(best, float((gap / xx.max()).min()))
    return best


@pytest.mark.parametrize("cls,name", [(DGCNN_cls, "dgcnn"), (GCNN_cls, "gcnn")])
def test_interaction_path_matches_reference(cls, name):
    g = load_golden("dgcnn.npz")
    model = make(cls)
    pts, label = synth.make_cloud(0)
    data = torch.from_numpy(pts).unsqueeze(0).to(dev())
    lbl = torch.tensor([label], device=dev())
    args = argparse.Namespace(model=name, softmax_type="modified", num_regions=32, interaction_batch_size=2)
    for ratio in g["ratios"]:
        tag = "ratio%d" % int(ratio * 100)
        logits = interaction.compute_order_interaction_logits(model, data, g["region_id"], g["pairs"], g[tag + "_contexts"], args)
        want = g["%s_%s_logits" % (tag, name)]
        assert logits.shape == want.shape
        got = logits.cpu().numpy()
        cond = np.zeros(1)
        if name == "gcnn":
            assert rel_err(got, want) < RTOL
            assert_close_elementwise(got, want)   # and element-wise, with an absolute floor (conftest.py)
        else:
            # DGCNN rebuilds its graph in feature space at every layer: a cloud that sits on a kNN near-tie
            # flips a neighbour under ANY rounding change (the reference's own float32 result is then far
            # from its float64 result).  Bar: 1e-4 relative, or 10x the reference's own float32
            # conditioning for such clouds (SURVEY.md §7 "index-valued kernels").
            scale = np.abs(want).max()
            cond = np.abs(want - g[tag + "_dgcnn_logits_fp64"]).max(axis=-1) / scale      # (P, 4C)
            err = np.abs(got - want).max(axis=-1) / scale
            assert np.median(err) < 1e-5
            for p, c in zip(*np.nonzero(err >= np.maximum(RTOL, 10 * cond))):
                # must be explained by a kNN near-tie in some layer of THIS cloud (gap between the 20th and
                # the 21st candidate below float32 resolution of the expanded-form distance), and stay small
                assert err[p, c] < 1e-3
                assert knn_min_margin(p, c, g, tag) < 2e-6, "cloud (%d,%d): error %.2e without a near-tie" % (p, c, err[p, c])
        inter = interaction.compute_order_interaction(logits, lbl, args)
        vmax = np.abs(hip_ops.reward(torch.from_numpy(want).reshape(-1, 10).to(dev()), label).cpu().numpy()).max()
        tol = RTOL if name == "gcnn" else max(RTOL, 40 * float(cond.max()))
        assert np.abs(inter - g["%s_%s_interaction" % (tag, name)]).max() < tol * vmax


@pytest.mark.parametrize("cls", [DGCNN_cls, GCNN_cls])
def test_compact_coalitions_equal_the_dense_forward_on_masked_clouds(cls):
    """iq_dgcnn_coalitions (kept points + <= 20 centre copies per coalition) against iq_dgcnn_forward on the
    materialised masked clouds: the same arithmetic on fewer rows, so agreement is to rounding of the mean pool.
    Covers no / few (< 20) / many / all points masked and several source clouds (cloud_of)."""
    model = make(cls)
    d = dev()
    rng = np.random.default_rng(3)
    clouds = torch.stack([torch.from_numpy(synth.make_cloud(i)[0]) for i in (0, 1)]).to(d)           # (2,1024,3)
    rid = torch.from_numpy(rng.integers(0, 32, size=(2, 1024)).astype(np.int32))
    rid[0, :12] = 40                                               # a 12-point region (fewer than 20 centre copies)
    rid[0, 12:] = torch.clamp(rid[0, 12:], max=31)
    centers = clouds.mean(dim=1)
    full = (1 << 41) - 1
    keep = [full, 0, full ^ (1 << 40), 1 << 40, 0x0f0f0f0f, (1 << 32) - 1, 1 << 5, full ^ 1, 0xaaaaaaaa | (1 << 40), 7]
    cloud_of = [0, 0, 0, 0, 0, 1, 1, 1, 1, 1]
    keep_t = hip_ops.masks_to_tensor(keep, d)
    co_t = torch.tensor(cloud_of, dtype=torch.int32, device=d)
    got = model.coalition_logits(clouds, centers, rid.to(d), keep_t, co_t, num_regions=41)
    dense = []
    for k, c in zip(keep, cloud_of):
        dense.append(hip_ops.mask_coalitions(clouds[c], rid[c].to(d), hip_ops.masks_to_tensor([k], d), centers[c].contiguous())[0])
    want = model.forward_points(torch.stack(dense))
    assert rel_err(got.cpu().numpy(), want.cpu().numpy()) < 1e-5


def test_interaction_shape_properties_at_bench_size():
    """BASELINE configs[3] shape (30 pairs x 100 contexts x 4 = 12 000 coalitions): a coalition's logits do not depend on
    what else is in the launch (bitwise), and the interaction of (i, j | S) equals that of (j, i | S) exactly."""
    model = make(DGCNN_cls)
    d = dev()
    pts, label = synth.make_cloud(0)
    data = torch.from_numpy(pts).unsqueeze(0).to(d)
    lbl = torch.tensor([label], device=d)
    region_id = hip_ops.region_assign(data[0].contiguous(), hip_ops.fps(data, 32)[0].contiguous()).cpu().numpy().astype(np.int64)
    rng = np.random.default_rng(1)
    all_pairs = np.array([[i, j] for i in range(32) for j in range(32) if j > i])
    pairs = all_pairs[rng.choice(len(all_pairs), size=30, replace=False)]
    ctx = np.stack([np.stack([rng.choice([r for r in range(32) if r not in pr], 15, replace=False) for _ in range(100)]) for pr in pairs])
    args = argparse.Namespace(model="dgcnn", softmax_type="modified", num_regions=32, interaction_batch_size=25)
    logits = interaction.compute_order_interaction_logits(model, data, region_id, pairs, ctx, args)          # (30, 400, 10)
    assert tuple(logits.shape) == (30, 400, 10) and torch.isfinite(logits).all()
    part = interaction.compute_order_interaction_logits(model, data, region_id, pairs[7:19], ctx[7:19], args)
    assert torch.equal(part, logits[7:19])
    swapped = interaction.compute_order_interaction_logits(model, data, region_id, pairs[:, ::-1].copy(), ctx, args)
    # rows 4k+1 / 4k+2 (S+i / S+j) trade places, rows 4k and 4k+3 are the same coalitions
    assert torch.equal(swapped[:, 0::4], logits[:, 0::4]) and torch.equal(swapped[:, 3::4], logits[:, 3::4])
    assert torch.equal(swapped[:, 1::4], logits[:, 2::4]) and torch.equal(swapped[:, 2::4], logits[:, 1::4])
    i1 = interaction.compute_order_interaction(logits, lbl, args)
    i2 = interaction.compute_order_interaction(swapped, lbl, args)
    assert i1.shape == (30, 100) and np.abs(i1 - i2).max() < 1e-6   # (v0 + v3) - v1 - v2 vs (v0 + v3) - v2 - v1 in float32


@pytest.mark.parametrize("cls", [DGCNN_cls, GCNN_cls])
def test_fused_edgeconv_is_bitwise_the_gemm_plus_gather(cls):
    """edge_fused_kernel (P/Q GEMM transposed onto the MFMA, P slice of the cloud in LDS, neighbourhood max from LDS) against
    the separate GEMM + gather_lds_kernel (twin "edge_gemm_lds") and GEMM + gather_max_kernel ("edge_gemm_l2"): the same products
    in the same order and the same maxima, so bit-identical logits - dense clouds and compact coalitions of every size class."""
    model = make(cls)
    d = dev()
    rng = np.random.default_rng(5)
    clouds = torch.stack([torch.from_numpy(synth.make_cloud(i)[0]) for i in (0, 1)]).to(d)
    rid = torch.from_numpy(rng.integers(0, 32, size=(2, 1024)).astype(np.int32)).to(d)
    centers = clouds.mean(dim=1)
    full = (1 << 32) - 1
    keep = [full, 0, 1, 3, 0xff, 0xffff, 0xffffff, full ^ 1, 0x0f0f0f0f, 0x55555555, 1 << 31, 0x3fffffff] * 3
    cloud_of = [i % 2 for i in range(len(keep))]
    keep_t = hip_ops.masks_to_tensor(keep, d)
    co_t = torch.tensor(cloud_of, dtype=torch.int32, device=d)

    def both():
        return (model.coalition_logits(clouds, centers, rid, keep_t, co_t, num_regions=32).clone(),
                model.forward_points(clouds).clone())
    fused = both()
    for name in ("edge_gemm_lds", "edge_gemm_l2"):
        split = tuning.tuned(name, both)
        assert torch.equal(fused[0], split[0]) and torch.equal(fused[1], split[1]), name


def test_knn_on_the_bf16_pipe_gives_the_graphs_of_the_fp32_mfma():
    """DGCNN's feature-space graphs with the inner products as three-term bf16 products (knn_kernel<.., BF3>, the default) against
    the fp32-MFMA kernels (twin "knn_fp32_mfma").  Both score within float32 rounding of the exact inner product and both hand every
    query whose boundary they cannot decide to the same exact re-ranking, so the neighbour SETS agree and with them the logits, bit
    for bit - on the op (random features with planted near-ties) and through the model (dense forward and compact coalitions)."""
    d = dev()
    rng = np.random.default_rng(17)
    fp32 = lambda fn: tuning.tuned("knn_fp32_mfma", fn)
    for c in (64, 128):
        x = rng.standard_normal((3, 1024, c)).astype(np.float32) + 1.5
        x[:, 1::4] = x[:, 0::4] + (rng.standard_normal((3, 256, c)) * 1e-4).astype(np.float32)
        xt = torch.from_numpy(x).to(d)
        a = np.sort(hip_ops.knn(xt, 20).cpu().numpy(), axis=-1)
        b = np.sort(fp32(lambda: hip_ops.knn(xt, 20)).cpu().numpy(), axis=-1)
        assert np.array_equal(a, b), (c, int((a != b).any(axis=-1).sum()))
    model = make(DGCNN_cls)
    clouds = torch.stack([torch.from_numpy(synth.make_cloud(i)[0]) for i in (5, 6)]).to(d)
    rid = torch.from_numpy(rng.integers(0, 32, size=(2, 1024)).astype(np.int32)).to(d)
    keep = [int(v) for v in rng.integers(0, 1 << 32, size=62)] + [(1 << 32) - 1, 1]
    keep_t = hip_ops.masks_to_tensor(keep, d)
    co_t = torch.tensor([i % 2 for i in range(len(keep))], dtype=torch.int32, device=d)

    def both():
        return (model.coalition_logits(clouds, clouds.mean(dim=1), rid, keep_t, co_t, num_regions=32).clone(),
                model.forward_points(clouds).clone())
    got, ref = both(), fp32(both)
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])


def test_forward_on_clouds_of_more_than_1024_points(oracle):
    """N = 1500 (the P slice of a cloud no longer fits the LDS budget: the L2 gather runs) against the CPU oracle."""
    rng = np.random.default_rng(11)
    x = torch.from_numpy(rng.uniform(-1, 1, size=(2, 1500, 3)).astype(np.float32))
    sd = synth.to_torch(synth.dgcnn_state_dict(0))
    with torch.no_grad():
        want = oracle.dgcnn_forward(sd, x.permute(0, 2, 1).contiguous(), 20, False)
    got = make(DGCNN_cls).forward_points(x.to(dev()))
    assert_close_elementwise(got.cpu().numpy(), want.numpy())



@pytest.mark.parametrize("cls", [DGCNN_cls, GCNN_cls])
def test_centre_multiplicity_around_k(cls):
    """The compact layout keeps the masked points as ONE centre row whose multiplicity min(M, 20) is applied when the kNN
    kernel writes the neighbour lists.  Coalitions with M = 1, 2, 19, 20, 21, 39, 41 and 1003 masked points (either side of
    k = 20, where the rule changes from "ranks among the 20" to "everything behind the centre falls out") against the
    dense forward on the materialised masked clouds."""
    model = make(cls)
    d = dev()
    cloud = torch.from_numpy(synth.make_cloud(2)[0]).to(d)                                            # (1024,3)
    sizes = [1, 1, 19, 20, 21]                                                                        # regions 0..4; region 5 = the rest
    rid = torch.full((1024,), 5, dtype=torch.int32)
    pos = 0
    perm = np.random.default_rng(4).permutation(1024)
    for r, n in enumerate(sizes):
        rid[perm[pos:pos + n]] = r
        pos += n
    full = (1 << 6) - 1
    masked_regions = [[0], [0, 1], [2], [3], [4], [2, 3], [3, 4], [0, 1, 2, 3, 4], [5], [5, 2]]       # M = 1, 2, 19, 20, 21, 39, 41, 62, 962, 981
    keep = [full ^ sum(1 << r for r in regs) for regs in masked_regions]
    clouds = cloud.unsqueeze(0)
    centers = clouds.mean(dim=1)
    rid_d = rid.unsqueeze(0).to(d)
    keep_t = hip_ops.masks_to_tensor(keep, d)
    got = model.coalition_logits(clouds, centers, rid_d, keep_t, None, num_regions=6)
    dense = torch.stack([hip_ops.mask_coalitions(cloud, rid.to(d), hip_ops.masks_to_tensor([k], d), centers[0].contiguous())[0]
                         for k in keep])
    want = model.forward_points(dense)
    assert rel_err(got.cpu().numpy(), want.cpu().numpy()) < 1e-5


@pytest.mark.parametrize("cls", [DGCNN_cls, GCNN_cls])
def test_layer1_graph_from_source_lists_is_bitwise_the_knn_kernel(cls):
    """dg_walk_kernel (layer-1 neighbours of a coalition = the first kept entries of its source point's sorted neighbour list,
    the centre counting min(M, 20) times) against knn_kernel<8> on the compact rows (twin "knn_compact"): the same
    neighbour sets, so bit-identical logits - two source clouds, coalitions from empty to full."""
    model = make(cls)
    d = dev()
    rng = np.random.default_rng(21)
    clouds = torch.stack([torch.from_numpy(synth.make_cloud(i)[0]) for i in (3, 4)]).to(d)
    rid = torch.from_numpy(rng.integers(0, 32, size=(2, 1024)).astype(np.int32))
    rid[1, :7] = 33                                                     # a 7-point region: M < 20 when only it is masked
    rid = rid.to(d)
    centers = clouds.mean(dim=1)
    full = (1 << 34) - 1
    keep = [int(x) | (1 << 33) for x in rng.integers(0, 1 << 32, size=44)] + [full, 0, full ^ (1 << 33), 1 << 33, 1, full ^ 1]
    cloud_of = [i % 2 for i in range(len(keep))]
    keep_t = hip_ops.masks_to_tensor(keep, d)
    co_t = torch.tensor(cloud_of, dtype=torch.int32, device=d)
    walk = model.coalition_logits(clouds, centers, rid, keep_t, co_t, num_regions=34).clone()
    with tuning.twin("knn_compact"):
        knn = model.coalition_logits(clouds, centers, rid, keep_t, co_t, num_regions=34).clone()
    assert torch.equal(walk, knn)


@pytest.mark.parametrize("n", [21, 24, 32])
def test_coalitions_on_clouds_of_barely_more_than_k_points(n, oracle):
    """Tiny clouds: a coalition then has fewer than 21 distinct rows AND fewer than 20 masked points, i.e. the top-21 list of the
    feature-space kNN holds empty slots while the cut behind the weighted centre row is decided by ranks.  (Round 5 found the
    exchange of the 21st slot copying a row into every empty slot there.)  Coalition path against the dense forward on the
    masked clouds and against the CPU oracle, DGCNN and GCNN."""
    d = dev()
    rng = np.random.default_rng(n)
    pts = torch.from_numpy(np.stack([synth.make_cloud(40 + i, num_points=n)[0] for i in range(2)]))
    clouds = pts.to(d)
    rid = torch.from_numpy(rng.integers(0, 8, size=(2, n)).astype(np.int32)).to(d)
    centers = clouds.mean(dim=1)
    keep = [255, 0, 1, 3, 0x0f, 0xf0, 0x55, 0xaa, 254, 127]
    cloud_of = [i % 2 for i in range(len(keep))]
    masked = torch.cat([hip_ops.mask_coalitions(clouds[c].contiguous(), rid[c].contiguous(), hip_ops.masks_to_tensor([k], d),
                                                centers[c].contiguous()) for k, c in zip(keep, cloud_of)])
    sd = synth.to_torch(synth.dgcnn_state_dict(0))
    for cls, fixed in ((DGCNN_cls, False), (GCNN_cls, True)):
        model = make(cls)
        got = model.coalition_logits(clouds, centers, rid, hip_ops.masks_to_tensor(keep, d),
                                     torch.tensor(cloud_of, dtype=torch.int32, device=d), num_regions=8).cpu().numpy()
        dense = model.forward_points(masked).cpu().numpy()
        with torch.no_grad():
            want = oracle.dgcnn_forward(sd, masked.cpu().permute(0, 2, 1).contiguous(), 20, fixed).numpy()
        scale = np.abs(want).max()
        assert np.abs(got - dense).max() / scale < 2e-5, (cls.__name__, np.abs(got - dense).max(axis=1) / scale)
        assert np.abs(got - want).max() / scale < 1e-4 and np.abs(dense - want).max() / scale < 1e-4
