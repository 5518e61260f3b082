"""GPU: the model kernels under weights other than ``synth.*_state_dict(0)`` (tests/weight_variants.py).

(a) PointNet against a float64 run of the CPU oracle, for seeds 1 and 2, dead channels (gamma = 0, bias < 0, > 0, +0.0, -0.0), a
    negative shift of every ReLU bias and a spread of the running variances: product coalition path (logits, feature transforms,
    arg-max rows), dense forward, wide entry (R = 128), and a cloud of 1024 points.  With e(x) = max |x - float64| / max |float64|,
    the bar is e(HIP) <= 4 e(float32 CPU oracle) + 1e-7, and never looser than 1e-4: the float32 oracle's own error measures how
    hard the case is, the factor 4 allows for another summation order over up to 1024 terms.  The arg-max rows are held by
    VALUE, every channel of every coalition: the float64 activation at the kernel's row is within 4 x the float32 oracle's
    largest error on that channel of the channel's float64 maximum, and the row is a kept one (or N, the centre).  The
    bit-for-bit relations of tests/test_chain_chunk96_gpu.py are repeated under every variant.
(b) Rescaling invariance, bit for bit, all five families: internal channels scaled by 2^k (|k| <= 12 and <= 6) and compensated in
    the next layer give the same logits (PointNet: feature transforms and arg-max rows too) as the base weights, on the product
    kernels and on their twins (TWINS below: tuning key 5 = 54 / 58; 56 / 64 for PointNet++ and PointConv).  tests/test_weight_variants_cpu.py
    shows the same on the CPU oracle, and that a compensation left out breaks it.
(c) PointNet++, PointConv, GCNN and DGCNN with dead channels and the negative shift: the bars of tests/test_fuzz_gpu.py against
    the dense HIP forward and the float32 oracle; PointNet++'s member-walk twin ("pn2_member_walk") bit for bit.  These run the `>= +0`
    assumptions of the integer maxima of csrc/iq_pointnet2.hip on rows that are exactly 0 and on a bias of -0.0.
    (DGCNN's 1e-2 here stays; tests/test_dgcnn_f64_gpu.py holds the same weights to the float64 bar on clouds with decidable graphs.)

Row counts of the PointNet coalitions: 1, 33, 65, 96, 97, 129, 193 and 200 (both sides of the 32 / 64 / 96 chunk edges, the empty and
the full coalition) among 16.  No four region sizes give all eight counts (exhaustive search), so the cloud has five regions of
1, 7, 24, 64 and 104 points."""
import numpy as np
import pytest
import torch

import probes
import weight_variants as V
from conftest import assert_close_elementwise
from interpret_quality_amd import hip_ops, synth
from interpret_quality_amd.tuning import tuned
from probes import rel_err

pytestmark = pytest.mark.gpu

PN_VARIANTS = ("seed1", "seed2", "dead", "negshift", "varspread")
NEED_ROWS = [1, 33, 65, 96, 97, 129, 193, 200]
SIZES = [1, 7, 24, 64, 104]


def dev():
    return torch.device("cuda:0")


# ---- the PointNet inputs: built once ------------------------------------------------------------------------------------------

_CASES = {}


def pn_small():
    """200 points in five regions, 16 keep masks: one per row count of NEED_ROWS (the first the empty coalition, the last the full
    one), 199 points and the centre, and seven more."""
    if "small" not in _CASES:
        d = dev()
        rid = np.repeat(np.arange(5), SIZES).astype(np.int32)
        np.random.default_rng(200).shuffle(rid)
        rows_of = lambda k: (lambda kept: kept + (kept < 200))(sum(SIZES[r] for r in range(5) if (k >> r) & 1))
        first = {}
        for k in range(32):
            first.setdefault(rows_of(k), k)
        first[200] = 31                                                      # the full coalition (mask 30: 199 points and the centre)
        keep = [first[r] for r in NEED_ROWS] + [30] + [k for r, k in sorted(first.items()) if r not in NEED_ROWS][:7]
        assert len(set(keep)) == 16 and [rows_of(k) for k in keep[:8]] == NEED_ROWS and keep[0] == 0
        data = torch.from_numpy(synth.make_cloud(41, 200)[0]).unsqueeze(0).to(d)
        _CASES["small"] = _case(data, rid, keep, 5)
    return _CASES["small"]


def pn_large():
    """1024 points, 8 regions of 128, three coalitions: 257 rows, 897 rows and the whole cloud."""
    if "large" not in _CASES:
        rid = np.repeat(np.arange(8), 128).astype(np.int32)
        np.random.default_rng(1024).shuffle(rid)
        data = torch.from_numpy(synth.make_cloud(42, 1024)[0]).unsqueeze(0).to(dev())
        _CASES["large"] = _case(data, rid, [0x03, 0x7f, 0xff], 8)
    return _CASES["large"]


def _case(data, rid, keep, nreg):
    d = data.device
    n = data.shape[1]
    center = torch.mean(data, dim=1).contiguous()
    rid_t = torch.from_numpy(rid).to(d).reshape(1, -1)
    keep_t = hip_ops.masks_to_tensor(keep, d)
    masked = hip_ops.mask_coalitions(data[0].contiguous(), rid_t[0].contiguous(), keep_t, center.reshape(3).contiguous())
    kept = np.stack([((k >> rid) & 1).astype(bool) for k in keep])                      # (B,N)
    return {"data": data, "center": center, "rid": rid_t, "keep": keep, "keep_t": keep_t, "nreg": nreg, "n": n, "kept": kept,
            "masked": masked, "masked_h": masked.cpu().numpy()}


def pn_wide():
    """The 200-point cloud as a game of 128 regions: six random coalitions, the full and the empty one."""
    if "wide" not in _CASES:
        d = dev()
        data = pn_small()["data"]
        r = 128
        rng = np.random.default_rng(128)
        rid = np.concatenate([np.arange(r), rng.integers(0, r, 200 - r)]).astype(np.int32)
        rng.shuffle(rid)
        member = rng.random((8, r)) < np.array([0.1, 0.3, 0.45, 0.5, 0.65, 0.9, 1.0, 0.0])[:, None]
        member[6, :] = True
        keep = np.stack([hip_ops.region_words(np.flatnonzero(m), r) for m in member])
        kw = hip_ops.wide_masks_to_tensor(keep, d)
        rid_t = torch.from_numpy(rid).to(d).reshape(1, -1)
        center = pn_small()["center"]
        masked = hip_ops.mask_coalitions_wide(data[0].contiguous(), rid_t[0].contiguous(), kw, center[0].contiguous(), r)
        _CASES["wide"] = {"data": data, "center": center, "rid": rid_t, "kw": kw, "r": r, "masked_h": masked.cpu().numpy()}
    return _CASES["wide"]


_RUNS = {}


def pn_run(variant, which):
    """Everything the HIP path gives for one variant and one case (product kernels), and the two oracle runs: computed once."""
    key = (variant, which)
    if key in _RUNS:
        return _RUNS[key]
    model, _ = probes.coalition_model("pointnet", dev(), variant)
    eng = model.engine()
    sd = V.variant("pointnet", variant)
    out = {}
    if which == "wide":
        c = pn_wide()
        out["logits"] = model.coalition_logits_wide(c["data"], c["center"], c["rid"], c["kw"], None, num_regions=c["r"]).cpu().numpy()
    else:
        c = pn_small() if which == "small" else pn_large()
        logits, tfp, crt = eng.coalition_logits(c["data"], c["center"], c["rid"], c["keep_t"], None, num_regions=c["nreg"],
                                                return_trans_feat=True, return_crt=True)
        out.update(logits_t=logits, tfp_t=tfp, logits=logits.cpu().numpy(), crt=crt.cpu().numpy(),
                   tf=tfp.index_select(1, eng.weights.unpack_index).reshape(-1, 64, 64).cpu().numpy())
        d_logits, d_tf, d_crt = model(c["masked"].permute(0, 2, 1).contiguous())
        out.update(dense_logits_t=d_logits, dense_logits=d_logits.cpu().numpy(), dense_tf=d_tf.cpu().numpy(), dense_crt=d_crt.cpu().numpy())
    for dt in ("float32", "float64"):
        o = V.oracle_forward("pointnet", sd, c["masked_h"], dt, return_aux=True)
        out[dt] = {"logits": o[0].numpy(), "tf": o[1].numpy(), "trunk": o[3]["trunk"].numpy()}
    _RUNS[key] = out
    return out


def assert_within_the_oracles_error(name, got, ref32, ref64):
    e_hip, e_ref = rel_err(got, ref64), rel_err(ref32, ref64)
    bar = min(4 * e_ref + 1e-7, 1e-4)
    print("%-44s e_hip %.3g  e_ref %.3g  e_hip / e_ref %.2f  (bar %.3g)" % (name, e_hip, e_ref, e_hip / max(e_ref, 1e-30), bar))
    assert np.isfinite(got).all(), name
    assert e_hip <= bar, "%s: e_hip %.3g above min(4 x %.3g + 1e-7, 1e-4)" % (name, e_hip, e_ref)


# ---- (a) PointNet against float64 ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", PN_VARIANTS)
def test_pointnet_logits_and_feature_transforms_against_float64(variant):
    for which in ("small", "large"):
        r = pn_run(variant, which)
        f32, f64 = r["float32"], r["float64"]
        tag = "%s N=%d " % (variant, 200 if which == "small" else 1024)
        assert_within_the_oracles_error(tag + "coalition logits", r["logits"], f32["logits"], f64["logits"])
        assert_within_the_oracles_error(tag + "coalition trans_feat", r["tf"], f32["tf"], f64["tf"])
        assert_within_the_oracles_error(tag + "dense logits", r["dense_logits"], f32["logits"], f64["logits"])
        assert_within_the_oracles_error(tag + "dense trans_feat", r["dense_tf"], f32["tf"], f64["tf"])
    r = pn_run(variant, "wide")
    assert_within_the_oracles_error("%s N=200 R=128 wide logits" % variant, r["logits"], r["float32"]["logits"], r["float64"]["logits"])


def crt_problems(crt, kept, h64, h32, n, centre_index=True):
    """crt (B,1024) rows; kept (B,N) bool; h64 / h32 (B,1024,N) pre-pool activations of the materialised clouds.  With
    ``centre_index`` (the coalition path) a row is a kept point or N = the centre, whose activations are those of any masked point;
    without (the dense forward on the materialised cloud) it is any of the N rows."""
    out = []
    for b in range(crt.shape[0]):
        idx = crt[b].astype(np.int64)
        if centre_index:
            masked = np.flatnonzero(~kept[b])
            legal = np.where(idx == n, len(masked) > 0, kept[b][np.minimum(idx, n - 1)] & (idx < n))
            if not legal.all():
                out.append("coalition %d: %d rows neither kept nor the centre" % (b, int((~legal).sum())))
                continue
            idx = np.where(idx == n, masked[0] if len(masked) else 0, idx)
        elif not ((idx >= 0) & (idx < n)).all():
            out.append("coalition %d: row outside [0, N)" % b)
            continue
        at = h64[b][np.arange(1024), idx]
        slack = 4 * np.abs(h32[b].astype(np.float64) - h64[b]).max(axis=1)
        short = h64[b].max(axis=1) - at - slack
        if (short > 0).any():
            c = int(short.argmax())
            out.append("coalition %d: %d channels below their maximum, worst channel %d by %.3g (slack %.3g)" % (
                b, int((short > 0).sum()), c, short[c] + slack[c], slack[c]))
    return out


@pytest.mark.parametrize("variant", PN_VARIANTS)
def test_pointnet_arg_max_rows_attain_the_float64_maximum(variant):
    for which, c in (("small", pn_small()), ("large", pn_large())):
        r = pn_run(variant, which)
        h64, h32 = r["float64"]["trunk"], r["float32"]["trunk"]
        assert r["crt"].shape == (len(c["keep"]), 1024)
        assert not crt_problems(r["crt"], c["kept"], h64, h32, c["n"]), which
        assert not crt_problems(r["dense_crt"], c["kept"], h64, h32, c["n"], centre_index=False), which


def test_the_arg_max_check_sees_a_row_dropped_from_the_pool():
    """The checker itself: the arg-max over all rows but the winner (what a kernel that drops a row would return) fails it on the
    channels that row wins, and a row that is not kept fails it whatever its value."""
    c, r = pn_small(), pn_run("seed1", "small")
    h64, h32 = r["float64"]["trunk"], r["float32"]["trunk"]
    b = 7                                                                    # the full coalition: every row kept
    assert c["kept"][b].all()
    drop = int(np.bincount(h64[b].argmax(axis=1)).argmax())                  # the row that wins the most channels
    second = np.where(np.arange(200)[None, :] == drop, -np.inf, h64[b]).argmax(axis=1)
    crt = r["crt"].copy()
    crt[b] = second
    assert crt_problems(crt, c["kept"], h64, h32, 200)
    crt = r["crt"].copy()
    crt[2, 5] = int(np.flatnonzero(~c["kept"][2])[0])                        # coalition 2 (64 kept): a masked point's own index
    assert crt_problems(crt, c["kept"], h64, h32, 200)


@pytest.mark.parametrize("variant", PN_VARIANTS)
def test_pointnet_bit_for_bit_relations(variant):
    """tests/test_chain_chunk96_gpu.py's: the product kernels against one n-tile per pass ("chain_l3_single"), against the dense forward on the
    materialised clouds, and a coalition alone against the same coalition in the batch."""
    model, _ = probes.coalition_model("pointnet", dev(), variant)
    eng = model.engine()
    c, r = pn_small(), pn_run(variant, "small")
    run = lambda keep_t: eng.coalition_logits(c["data"], c["center"], c["rid"], keep_t, None, num_regions=c["nreg"], return_trans_feat=True)
    one, tf_one = tuned("chain_l3_single", lambda: run(c["keep_t"]))
    assert torch.equal(one, r["logits_t"]) and torch.equal(tf_one, r["tfp_t"])
    assert torch.equal(r["dense_logits_t"], r["logits_t"])
    for i, k in enumerate(c["keep"]):
        alone, tf_alone = run(hip_ops.masks_to_tensor([k], dev()))
        assert torch.equal(alone[0], r["logits_t"][i]) and torch.equal(tf_alone[0], r["tfp_t"][i]), "coalition %d" % i
    big = pn_run(variant, "large")
    assert torch.equal(big["dense_logits_t"], big["logits_t"])


# ---- (b) rescaling invariance, bit for bit ------------------------------------------------------------------------------------------

FAMILY_CASE = {"pointnet2": probes.CoalitionCase("pointnet2", 160, 8, 1, 12, 51), "pointconv": probes.CoalitionCase("pointconv", 100, 8, 1, 12, 52),
               "gcnn": probes.CoalitionCase("gcnn", 40, 8, 1, 12, 53), "dgcnn": probes.CoalitionCase("dgcnn", 40, 8, 1, 12, 54)}
TWINS = {"pointnet": (None, "chain_l3_fp32", "chain_l3_single"), "pointnet2": (None, "group_fp32", "group_fp32_chunk64"),
         "pointconv": (None, "group_fp32", "group_fp32_chunk64"), "gcnn": (None,), "dgcnn": (None,)}     # None: the product kernels


def _pointnet_outputs(variant):
    model, _ = probes.coalition_model("pointnet", dev(), variant)
    out = []
    for c in (pn_small(), pn_large()):
        out += list(model.engine().coalition_logits(c["data"], c["center"], c["rid"], c["keep_t"], None, num_regions=c["nreg"],
                                                    return_trans_feat=True, return_crt=True))
        out += list(model(c["masked"].permute(0, 2, 1).contiguous()))
    w = pn_wide()
    out.append(model.coalition_logits_wide(w["data"], w["center"], w["rid"], w["kw"], None, num_regions=w["r"]))
    return out


def _family_outputs(family, variant):
    got, dense, _, _ = probes.run_coalition_case(FAMILY_CASE[family], dev(), oracle_cap=0, variant=variant)
    return [torch.from_numpy(got), torch.from_numpy(dense)]


@pytest.mark.parametrize("family", V.FAMILIES)
def test_rescaled_channels_give_the_same_bits(family):
    outputs = _pointnet_outputs if family == "pointnet" else (lambda v: _family_outputs(family, v))
    for key in TWINS[family]:
        base = tuned(key, lambda: outputs("base"))
        assert all(torch.isfinite(t.float()).all() for t in base)
        for variant in ("rescaled12", "rescaled6"):
            got = tuned(key, lambda: outputs(variant))
            assert len(got) == len(base)
            for i, (g, b) in enumerate(zip(got, base)):
                assert torch.equal(g, b), "%s, twin %s, output %d: max |diff| %.3g of %.3g" % (
                    variant, key, i, (g.double() - b.double()).abs().max().item(), b.double().abs().max().item())


# ---- (c) dead, zero and signed-zero channels in the grouped families ---------------------------------------------------------

@pytest.mark.parametrize("variant", ("dead", "negshift"))
@pytest.mark.parametrize("family", ("pointnet2", "pointconv", "gcnn", "dgcnn"))
def test_grouped_families_with_dead_and_zero_channels(family, variant):
    case = FAMILY_CASE[family]
    got, dense, want, _ = probes.run_coalition_case(case, dev(), variant=variant)
    assert got.shape == (case.b, 10) and np.ptp(want, axis=0).max() > 0
    print("%s %s: vs dense %.3g, vs oracle %.3g" % (family, variant, probes.rel_max_err(got, dense), probes.rel_max_err(got, want)))
    problems = probes.coalition_problems(family, got, dense, want)
    assert not problems, problems
    if family != "dgcnn":
        assert_close_elementwise(got, want)
    if family == "pointnet2":                                   # the member-walk twin against the region tables
        walk = tuned("pn2_member_walk", lambda: probes.run_coalition_case(case, dev(), oracle_cap=0, variant=variant)[0])
        assert probes.bitwise_equal(walk, got)
