#!/bin/bash
# Copy a round's GPU evidence (scripts/gpu_round.sh <tag>) from $OUT (default bench_out/) into profiles/.
# (referenced from DESIGN.md section 9: the evidence files each round commits)
T=$1; OUT=${OUT:-$PWD/bench_out}
cp $OUT/bench_$T.json profiles/${T}_bench_fpfh_line.json
for w in shot match iss harris harris6d config1 fastnormals demand scans8 dense; do cp $OUT/bench_${w}_$T.json profiles/${T}_bench_${w}_line.json; done
cp $OUT/prof_$T/run_kernel_stats.csv profiles/${T}_kernel_stats.csv
cp $OUT/prof_iss_$T/run_kernel_stats.csv profiles/${T}_iss_kernel_stats.csv
cp $OUT/prof_match_$T/run_kernel_stats.csv profiles/${T}_match_kernel_stats.csv
cp $OUT/pmc_$T/summary.txt profiles/${T}_pmc_summary.txt
cp $OUT/pmc_$T/pmc_normals_stage.json profiles/pmc_normals_stage.json
cp $OUT/pmc_$T/pmc_normals_chain.json profiles/pmc_normals_chain.json
cp $OUT/t_$T.log profiles/${T}_pytest_gpu.log
[ -f $OUT/prof_dense_$T/run_kernel_stats.csv ] && cp $OUT/prof_dense_$T/run_kernel_stats.csv profiles/${T}_dense_normals_kernel_stats.csv
[ -f $OUT/prof_dense_$T.log ] && grep -E "^(dense)" $OUT/prof_dense_$T.log > profiles/${T}_dense_normals_only.txt
