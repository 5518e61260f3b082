"""CPU: what tests/test_f64_families_gpu.py relies on, shown on the CPU oracle alone (tests/f64_cases.py).

* For every (case, variant) the float32 and the float64 oracle make identical discrete choices - FPS centroids and ball-query
  groups (PointNet++), FPS centroids and kNN sets (PointConv), the xyz kNN sets (GCNN) - so e_ref is rounding error and nothing
  else.  No seed had to be changed for this: the seeds of ``f64_cases.cases`` are the first ones tried.
* 1e-8 <= e_ref <= 2.5e-5 and 4 e_ref + 1e-7 < 1e-4: the 1e-4 clamp is never the active bar, and e_ref is no accident of a case on
  which the float32 oracle happens to be exact.
* The float64 logits move over the coalitions of a case (ptp > 1e-3 of max |logit|): a route that ignored the mask would fail.
* The checker can fail: the float32 oracle on weights that lost their third bf16 term (``trunc16``; the grouped layers alone, the
  heads alone, both) is above the bar against float64 of the true weights, and so are the float32 logits with 1e-5 max |logit|
  added to one entry.
"""
import numpy as np
import pytest

import f64_cases as F
import weight_variants as V


@pytest.mark.parametrize("pair", F.PAIRS, ids=F.pair_id)
def test_both_precisions_make_the_same_choices_and_the_bar_is_live(pair):
    family, case, variant = pair
    i = F.inputs(case)
    assert i["kept"][0].all() and not i["kept"][-1].any()
    assert np.array_equal(i["masked"][0], i["clouds"][i["cloud_of"][0]])
    assert (i["masked"][-1] == i["centers"][i["cloud_of"][-1]][None]).all()
    run = F.oracle_run(family, case, variant)
    f64 = run["f64"]
    spread = np.ptp(f64, axis=0).max() / np.abs(f64).max()
    print("%-48s e_ref %.3g  bar %.3g  ptp over coalitions %.3g of max |logit|" % (F.pair_id(pair), run["e_ref"], run["bar"], spread))
    assert np.isfinite(f64).all() and np.isfinite(run["f32"]).all()
    assert not F.choice_mismatches(run), F.choice_mismatches(run)
    assert 1e-8 <= run["e_ref"] <= 2.5e-5
    assert run["bar"] == F.FACTOR * run["e_ref"] + 1e-7 < F.CLAMP
    assert spread > 1e-3


def test_the_overflow_case_exceeds_the_pair_table_and_the_others_do_not():
    """What the GPU test says about which PointNet++ case runs sa1's widest scale on the grouped MLP, counted on the host."""
    for case in F.cases("pointnet2"):
        rows, cap = F.pn2_pair_rows(case)
        loose, _ = F.pn2_pair_rows(case, shave=-1e-5)
        print("%-40s pair rows at radius 0.4: %d to %d, capacity %d" % (case.id, rows, loose, cap))
        if case.name == "overflow":
            assert rows > cap
        else:
            assert loose <= cap


@pytest.mark.parametrize("family", F.FAMILIES)
def test_a_lost_bf16_term_and_a_perturbed_logit_are_above_the_bar(family):
    case = F.stress_base(family)
    run = F.oracle_run(family, case, "base")
    sd = V.variant(family, "base")
    masked = F.inputs(case)["masked"]
    group, heads = F.BF16_GROUP_LAYERS[family], F.BF16_HEAD_LAYERS[family]
    assert all(k in sd for k in group + heads)
    for name, keys in (("group layers", group), ("heads", heads), ("both", group + heads)):
        got = V.oracle_forward(family, F.trunc16(sd, keys), masked, "float32").numpy()
        e = F.rel_err(got, run["f64"])
        print("%s %-12s e %.3g  bar %.3g  e / bar %.2f" % (family, name, e, run["bar"], e / run["bar"]))
        assert e > run["bar"], (family, name, e, run["bar"])
    bumped = run["f32"].copy()
    bumped[1, 3] += 1e-5 * np.abs(run["f64"]).max()
    assert F.rel_err(bumped, run["f64"]) > run["bar"]


def test_trunc16_keeps_sixteen_significant_bits():
    w = np.array([1.0, 1.0 + 2.0 ** -16, 1.0 + 2.0 ** -16 + 2.0 ** -23, 1.0 + 3 * 2.0 ** -16, -3.1415927, 1e-3, 255.99999], dtype=np.float32)
    got = F.trunc16({"w": w, "other": w.copy()}, ["w"])
    assert np.array_equal(got["other"], w) and got["w"].dtype == np.float32
    assert not (got["w"].view(np.uint32) & 0xFF).any()
    # ties to even at 1 + 2^-16 (down) and 1 + 3 2^-16 (up), nearest just above the tie
    assert got["w"][:4].tolist() == [1.0, 1.0, 1.0 + 2.0 ** -15, 1.0 + 2.0 ** -14]
    assert np.abs(got["w"].astype(np.float64) - w).max() <= np.abs(w.astype(np.float64)).max() * 2.0 ** -16
    assert (np.abs(got["w"].astype(np.float64) - w) <= np.abs(w.astype(np.float64)) * 2.0 ** -16).all()
