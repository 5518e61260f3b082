#!/usr/bin/env python3
"""Randomised probe of the hot path's boundary (GPU): shap_sampling_all_regions_batch, compute_order_interaction_logits and the
region assignment behind them on random cloud sizes (8-4096), region counts (1-64), permutation counts / batch sizes, both softmax
types - the HIP path (interpret_quality_amd.final_common / interaction) against the CPU oracle's restatement of the reference loop.

    python tests/fuzz_hotpath.py [seed] [seconds]

PointNet (the oracle's restatement of the loop is PointNet's; the other families' coalition paths: tests/fuzz_sizes.py).  Prints every case that
raises or disagrees (> 1e-4 of the largest logit / Shapley value) and a final count.  The case generator and the checks live in
tests/probes.py; a seeded slice of them, with the boundary sizes spelled out, runs in the suite as tests/test_fuzz_gpu.py.
Test infrastructure (imports oracle/); not collected by pytest."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

import probes

d = torch.device("cuda:0")
rng = np.random.default_rng(int(sys.argv[1]) if len(sys.argv) > 1 else 0)
budget = float(sys.argv[2]) if len(sys.argv) > 2 else 60.0
t0, ncase, nbad = time.time(), 0, 0
while time.time() - t0 < budget:
    case = probes.random_hotpath_case(rng)
    desc = "pointnet N=%d R=%d S=%d bs=%d %s" % (case.n, case.r, case.s, case.bs, case.sm)
    try:
        res = probes.run_hotpath_case(case, d)
        ncase += 1
        if probes.hotpath_problems(res):
            nbad += 1
            geom_ok, e_l, e_p, e_i = probes.hotpath_errors(res)
            print("MISMATCH %s: geometry %s, logits %.2g, phi %.2g (max |phi| %.3g), interaction logits %.2g" % (
                desc, "ok" if geom_ok else "BAD", e_l, e_p, np.abs(res["want_phi"]).max(), e_i), flush=True)
    except Exception as e:   # noqa: BLE001 - a probe: report and go on
        ncase += 1
        print("%s: %s: %s" % (desc, type(e).__name__, str(e)[:160]), flush=True)
print("cases %d, mismatches %d" % (ncase, nbad))
