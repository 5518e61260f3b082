#!/usr/bin/env python3
"""Exact Shapley values and all-order interactions of every selected cloud by full enumeration (the reference has no such
script: it samples, final_shapley_value.py).  Flags of final_shapley_value.py plus --num_regions (default 16, at most 24).
Thin driver: all logic lives in interpret_quality_amd/, all arithmetic in libiq_hip.so."""
from interpret_quality_amd.exact_stage import main

from interpret_quality_amd.exact_stage import exact_one_cloud, make_args, run  # noqa: F401,E402

if __name__ == "__main__":
    main()
