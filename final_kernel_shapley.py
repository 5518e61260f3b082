#!/usr/bin/env python3
"""Region Shapley values of every selected cloud by the regression (KernelSHAP) estimator with paired sampling (the reference has
no such script: it walks sampled permutations, final_shapley_value.py).  Flags of final_shapley_value.py plus --num_regions
(2 to 64), --samples, --unpaired, --gram sampled|analytic and --compare_exact.
Thin driver: all logic lives in interpret_quality_amd/, all arithmetic in libiq_hip.so."""
from interpret_quality_amd.kernel_stage import main

from interpret_quality_amd.kernel_stage import kernel_one_cloud, make_args, run  # noqa: F401,E402

if __name__ == "__main__":
    main()
