#!/usr/bin/env python3
"""Region Shapley values of every selected cloud while the linearity / planarity / scattering of every region is pushed up or down,
for MORE than 64 regions, up to one region per point: final_smoothness_center_enum_all.py on the region ids and permutations
final_wide_shapley.py wrote for the same --num_regions (65 .. 1024, default 128).  Flags of final_wide_shapley.py plus
--num_samples K (the first K permutations, default 100); that stage's artefacts without all_logits.pt, epochs sharded over the
ranks.  Thin driver: all logic lives in interpret_quality_amd/, all arithmetic in libiq_hip.so."""
from interpret_quality_amd.wide_smoothness_stage import main

from interpret_quality_amd.wide_smoothness_stage import make_args, run  # noqa: F401,E402

if __name__ == "__main__":
    main()
