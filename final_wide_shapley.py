#!/usr/bin/env python3
"""Region Shapley values of every selected cloud for MORE than 64 regions, up to one region per point (the reference edits
NUM_REGIONS for this: tools/final_util.py:20-22).  Flags of final_shapley_value.py plus --num_regions (65 .. 1024, default 128;
--num_regions 1024 = the number of points: the per-point game) and --num_samples_save; stage 1's artefacts, in the experiment
folder of that region count.  Thin driver: all logic lives in interpret_quality_amd/, all arithmetic in libiq_hip.so."""
from interpret_quality_amd.wide_stage import main

from interpret_quality_amd.wide_stage import cal_region_id, generate_all_orders, make_args, run  # noqa: F401,E402

if __name__ == "__main__":
    main()
