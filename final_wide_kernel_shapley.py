#!/usr/bin/env python3
"""Region Shapley values of every selected cloud of a WIDE game (65 .. 1024 regions, up to one region per point) by the regression
(KernelSHAP) estimator with paired sampling and the analytic Gram matrix (the reference has no such script).  Flags of
final_shapley_value.py plus --num_regions (65 .. 1024, default 128), --coalitions dense|compact, --samples, --unpaired and
--draw stream|counter (how the rows are drawn: NumPy's MT19937 stream, the default, or counter-based by seed, cloud and row);
2 .. 64 regions: final_kernel_shapley.py.
Thin driver: all logic lives in interpret_quality_amd/, all arithmetic in libiq_hip.so."""
from interpret_quality_amd.wide_kernel_stage import main

from interpret_quality_amd.wide_kernel_stage import kernel_one_cloud, make_args, run  # noqa: F401,E402

if __name__ == "__main__":
    main()
