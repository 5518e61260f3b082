#!/usr/bin/env python3
"""One dense layer per branch of the dispatch (csrc/iq_linear_plan.h: plan_linear), for a kernel trace of a 256-CU board:

    rocprofv3 --kernel-trace -- python tools/linear_trace_cases.py

``hip_ops.linear`` (the C entry iq_linear: fit_tiles, no tile_nu, no m_dev) is called once per case; together the cases launch
every kernel instantiation launch_linear has and take every branch of the round rule (a round = 2 x 256 workgroups of 128 rows).
Two libraries that plan alike give the same ordered list of (kernel, grid, workgroup size); ``IQ_LIBPATH`` selects the library.
The row counts are the smallest ones ``tests/cpp/linear_plan_check.cpp --branches`` prints, or the sizes the layers were measured
at.  Prints the number of cases.  (Not the flagship workload: that is bench.py.)"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from interpret_quality_amd import hip_ops  # noqa: E402

ROUND = 2 * 256
# (M, cin, cout, bf16x3 image): what plan_linear gives on 256 CUs
CASES = [
    (33000, 512, 256, True),                        # below one round: 32-row tiles throughout
    (33000, 1024, 512, True),                       # below two rounds: 64-row tiles throughout
    (33000, 256, 4096, True),                       # 8.06 rounds: 128-row tiles + the last sixteenth of a round on 32-row tiles
    ((2 * ROUND + 3 * ROUND // 8) * 128 - 5, 64, 256, True),    # a third round three eighths full: 128-row + 64-row tail
    ((2 * ROUND + 3 * ROUND // 4) * 128 + 9, 64, 256, True),    # three quarters full: 128-row tiles throughout
    (2 * ROUND * 128, 64, 256, True),               # whole rounds exactly
    (100, 40, 256, True),                           # ragged k: 32-row tiles,
    (70000, 40, 256, True),                         # 64-row tiles,
    (140000, 40, 256, True),                        # 128-row + 32-row tail,
    ((2 * ROUND + 200) * 128 - 5, 40, 256, True),   # 128-row + 64-row tail
    (1000, 32, 320, True),                          # 256 + 64 outputs: bf16x3 block, the rest on pn_linear_kernel<2, 1, 4, 1>
    (524033, 32, 320, True),                        # the rest on 256-row LDS tiles (2048 of them)
    (524033, 32, 64, False),                        # pn_gemm_lds_kernel<2, false, 1>
    (524033, 32, 128, False),                       # pn_gemm_lds_kernel<4, false, 1>
    (262017, 32, 320, False),                       # pn_gemm_lds_kernel<5, false>
    (262017, 32, 256, False),                       # pn_gemm_lds_kernel<4, false>, one column block: (tiles, blocks) grid
    (130945, 32, 512, False),                       # two column blocks: flat grid
    (4096, 32, 128, False),                         # pn_gemm_lds_kernel<2, false>
    (100, 32, 128, False),                          # pn_linear_kernel<2, 2, 2, 2>
    (100, 256, 40, False),                          # pn_linear_kernel<2, 1, 4, 1>
]


def run(cases=CASES, keep=None):
    """Calls hip_ops.linear once per case; ``keep(case, out)`` sees every output before it is dropped."""
    dev = torch.device("cuda:0")
    layers = {}
    for case in cases:
        m, cin, cout, bf3 = case
        if (cin, cout, bf3) not in layers:
            rng = np.random.default_rng(1000 * cin + cout)
            w = (rng.standard_normal((cout, cin)) / np.sqrt(cin)).astype(np.float32)
            layers[(cin, cout, bf3)] = hip_ops.PackedLinear(w, rng.standard_normal(cout).astype(np.float32), dev, bf3=bf3)
        x = torch.randn((m, cin), dtype=torch.float32, device=dev, generator=torch.Generator(dev).manual_seed(m))
        out = hip_ops.linear(x, layers[(cin, cout, bf3)], 1)
        torch.cuda.synchronize()
        if keep is not None:
            keep(case, out)
        del x, out
    return len(cases)


if __name__ == "__main__":
    print(run())
