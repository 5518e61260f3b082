#!/usr/bin/env python3
"""Region Shapley values of every selected cloud for EVERY class (or --classes 0,3,7) from one pass over the game's coalitions (the
reference scores the ground-truth label only).  Runs on the folder stage 1 wrote for --num_regions (2 .. 1024, default 32:
final_shapley_value.py up to 64 regions, final_wide_shapley.py above).  Flags of final_shapley_value.py plus --estimator
permutation|kernel, --classes, --num_samples, above 64 regions --route and --coalitions, for the kernel estimator --samples, --draw
and --seed.  One rank.
Thin driver: all logic lives in interpret_quality_amd/, all arithmetic in libiq_hip.so."""
from interpret_quality_amd.class_stage import main

from interpret_quality_amd.class_stage import class_one_cloud, make_args, run  # noqa: F401,E402

if __name__ == "__main__":
    main()
