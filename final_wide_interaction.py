#!/usr/bin/env python3
"""Multi-order interactions of every selected cloud for MORE than 64 regions, up to one region per point: the pairs and contexts
of final_gen_pair.py, the logits of final_point_binary_interaction_logits.py and the interactions of final_cal_interactions.py in
one run, on the region ids final_wide_shapley.py wrote for the same --num_regions (65 .. 1024, default 128).  Flags of those three
scripts plus --num_regions and --transform_params FILE.npy (also evaluate the pose of --mode given there, into <mode>_adv/) or
--adv_pose sweep (that pose = the lowest-reward pose of the sweep final_wide_pose.py --mode wrote).
Thin driver: all logic lives in interpret_quality_amd/, all arithmetic in libiq_hip.so."""
from interpret_quality_amd.wide_interaction_stage import main

from interpret_quality_amd.wide_interaction_stage import draw, evaluate, make_args, run  # noqa: F401,E402

if __name__ == "__main__":
    main()
