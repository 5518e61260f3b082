#!/bin/bash
# The wide pipeline (65 .. 1024 regions): stage 1, the three pose sweeps, the smoothness stage and the multi-order interactions
# at the sweep's adversarial pose.  Variables as in scripts/exp_shapley.sh: pass --synthetic / --num_regions R / --sampler device through EXTRA;
# prefix with "torchrun --nproc-per-node N" via LAUNCH to shard the pose and smoothness stages over N GPUs (stage 1 and the
# interaction stage run on rank 0).
model="pointnet";
dataset="shapenet";
device_id=0;
LAUNCH=${LAUNCH:-python}
EXTRA=${EXTRA:-}
$LAUNCH final_wide_shapley.py --model=$model --dataset=$dataset --device_id=$device_id $EXTRA
$LAUNCH final_wide_pose.py --mode=trans --model=$model --dataset=$dataset --device_id=$device_id $EXTRA
$LAUNCH final_wide_pose.py --mode=rotate --model=$model --dataset=$dataset --device_id=$device_id $EXTRA
$LAUNCH final_wide_pose.py --mode=scale --model=$model --dataset=$dataset --device_id=$device_id $EXTRA
$LAUNCH final_wide_smoothness.py --model=$model --dataset=$dataset --device_id=$device_id $EXTRA
$LAUNCH final_wide_interaction.py --adv_pose=sweep --mode=rotate --model=$model --dataset=$dataset --device_id=$device_id $EXTRA
