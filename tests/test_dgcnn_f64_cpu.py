"""CPU: what tests/test_dgcnn_f64_gpu.py relies on, shown on the CPU oracle alone (tests/dgcnn_f64_cases.py).

* Every recorded seed is decidable for its variant: the smallest margin over the queries of the four graphs (xyz, x1, x2, x3) of
  every masked cloud, in the float64 run, is at least MARGIN = 3e-5.  No listed shape had to be dropped: the share of cases left out
  is zero (the stress size has one seed per weight variant, see ``dgcnn_f64_cases.SEARCHES``).  That includes the stress shape
  under scale 0.5, scale 2.0 and a translation of 0.5 (``dgcnn_f64_cases.POSE``), each with a seed found at 40 points.
* The float32 and the float64 oracle make the same canonical neighbour sets in all four graphs, so e_ref is rounding error and
  nothing else; 1e-8 <= e_ref, and 4 e_ref + 1e-7 < 1e-4: the clamp is never the active bar.
* The same for the two coalitions of the centre-multiplicity test (M around k, and the empty coalition).
* ``find_seed`` returns the recorded seed when started just below it, and the margin sees a planted near tie.
* The checker can fail: the float32 oracle on weights that lost their third bf16 term (``f64_cases.trunc16``) is above the bar on the
  stress case against float64 of the true weights - conv5 and the heads, and the EdgeConv layers conv2 - conv4 (what they stand
  for: ``dgcnn_f64_cases.EDGE_LAYERS``).  The truncated EdgeConv weights move the features the graphs of layers 3 - 4 are built
  from, so that part first asserts that the float64 run with them still makes the unchanged graphs, and stays decidable.
"""
import numpy as np
import pytest

import dgcnn_f64_cases as D
import f64_cases as F
import weight_variants as V

HEAD_LAYERS, EDGE_LAYERS = D.HEAD_LAYERS, D.EDGE_LAYERS


def check_run(tag, run):
    margin, graph = D.min_margin(run)
    print("%-44s smallest margin %.3g (%s)  e_ref %.3g  bar %.3g" % (tag, margin, graph, run["e_ref"], run["bar"]))
    assert np.isfinite(run["f64"]).all() and np.isfinite(run["f32"]).all()
    assert margin >= D.MARGIN, (tag, margin, graph)
    assert F.choice_mismatches(run) == []
    assert 1e-8 <= run["e_ref"]
    assert run["bar"] == F.FACTOR * run["e_ref"] + 1e-7 < F.CLAMP


@pytest.mark.parametrize("pair", D.pairs(), ids=D.pair_id)
def test_the_recorded_seed_is_decidable_and_both_precisions_make_the_same_graphs(pair):
    case, variant = pair
    i = F.inputs(case)
    assert case.spec[1:5] == D.SHAPES[case.name][0] and case.wide == D.SHAPES[case.name][1]
    assert i["kept"][0].all() and not i["kept"][-1].any()
    run = D.oracle_run(case, variant)
    check_run(D.pair_id(pair), run)
    spread = np.ptp(run["f64"], axis=0).max() / np.abs(run["f64"]).max()
    assert spread > 1e-3, spread            # the logits move over the coalitions: a route that ignored the mask would fail
    assert np.isinf(run["margins"]["x3"][-1]).all()          # the empty coalition: every row the centre, nothing to decide


def test_the_multiplicity_coalitions_are_decidable():
    case = D.stress_case()
    inp = D.multiplicity_inputs(case)
    masked = (~inp["kept"]).sum(axis=1)
    assert D.K - 1 <= masked[0] <= D.K + 1 and masked[1] == case.spec.n
    assert (inp["masked"][1] == inp["centers"][0][None]).all()
    check_run("multiplicity M = %d, %d" % tuple(masked), D.oracle_run(case, "base", multiplicity=True))


def test_find_seed_returns_the_recorded_seed_and_the_margin_sees_a_planted_tie():
    seed = D.SEEDS["edge", "base"]
    assert D.find_seed("edge", ("base",), seed, limit=1) == seed
    rng = np.random.default_rng(0)
    x = rng.standard_normal((1, 30, 8))
    rows = np.zeros((1, 30), dtype=bool)
    d = ((x[0, 0] - x[0]) ** 2).sum(-1)
    order = np.argsort(d)
    b = x[0, order[D.K]]
    before = D.graph_margins(x, rows)[0, 0]
    x[0, order[D.K]] = x[0, 0] + (b - x[0, 0]) * np.sqrt(d[order[D.K - 1]] / d[order[D.K]]) * (1 + 1e-7)   # the 21st at the 20th's distance
    after = D.graph_margins(x, rows)[0, 0]
    assert before > 1e-4 > D.MARGIN > after >= 0, (before, after)
    # copies of one row that straddle the boundary: the exact tie among them is no tie, the kept rows next to them decide
    y = rng.standard_normal((1, 30, 8))
    rows[0, 5:] = True
    y[0, 5:] = y[0, 5]
    m = D.graph_margins(y, rows)[0]
    dq = ((y[0, 0] - y[0]) ** 2).sum(-1)
    near = np.abs(dq[1:5] - dq[5]).min() / (2 * ((y[0, 0] ** 2).sum() + max(dq[5], dq[1:5][np.abs(dq[1:5] - dq[5]).argmin()])))
    assert np.isclose(m[0], near, rtol=1e-12) and m[0] > 0
    sets = D.canonical_sets(np.array([[list(range(10, 30))] * 30]), rows)
    assert sets[0, 0].sum() == 1 and sets[0, 0, 5]


def test_a_lost_bf16_term_is_above_the_bar():
    case = D.stress_case()
    run = D.oracle_run(case, "base")
    sd = V.variant("dgcnn", "base")
    inp = F.inputs(case)
    assert all(k in sd for k in HEAD_LAYERS + EDGE_LAYERS)
    # the truncated EdgeConv weights leave every graph of the float64 run as it was, and decidable
    edge64 = D.run_inputs(inp, F.trunc16(sd, EDGE_LAYERS), only_f64=True)
    for (name, got), (_, want) in zip(edge64["choices"]["float64"], run["choices"]["float64"]):
        assert np.array_equal(got, want), name
    print("EdgeConv layers truncated: smallest margin %.3g (%s)" % D.min_margin(edge64))
    assert D.decidable(edge64)
    for name, keys in (("conv5 and heads", HEAD_LAYERS), ("EdgeConv 2-4", EDGE_LAYERS), ("both", HEAD_LAYERS + EDGE_LAYERS)):
        got = V.oracle_forward("dgcnn", F.trunc16(sd, keys), inp["masked"], "float32").numpy()
        e = F.rel_err(got, run["f64"])
        print("%-16s e %.3g  bar %.3g  e / bar %.2f" % (name, e, run["bar"], e / run["bar"]))
        assert e > run["bar"], (name, e, run["bar"])
    bumped = run["f32"].copy()
    bumped[1, 3] += 1e-5 * np.abs(run["f64"]).max()
    assert F.rel_err(bumped, run["f64"]) > run["bar"]
