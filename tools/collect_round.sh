#!/bin/bash
# Everything a round commits under profiles/, in one gpurun call from the repo root: tools/collect_round.sh r06
# (kernel trace + PMC traffic of bench.py, the two-stream timeline, the side workloads, SQ counters of the attention kernels, the convergence run,
# the default bench line).  Outputs under gpurun_out/round_<R>/.
set -u
R=${1:-rXX}
D=gpurun_out/round_$R
mkdir -p $D
bash tools/collect_profiles.sh $R > $D/collect.log 2>&1
cp gpurun_out/prof_$R/${R}_* $D/
KT=$(find gpurun_out/prof_$R/kt -name "*_results.db" | head -1)
python tools/timeline.py $KT $D/${R}_timeline.md > /dev/null 2>&1
bash tools/collect_side.sh $R > $D/side.log 2>&1
cp gpurun_out/prof_${R}_cfg4/${R}_cfg4_* gpurun_out/prof_${R}_cfg5/${R}_cfg5_* $D/ 2>/dev/null
bash tools/sq_one.sh seq seq_ python tools/seq_attn_one.py > $D/sq_seq.log 2>&1; cp gpurun_out/sq_seq/sq.md $D/${R}_sq_seq.md
bash tools/sq_one.sh win win_ python tools/win_bias_one.py > $D/sq_win.log 2>&1; cp gpurun_out/sq_win/sq.md $D/${R}_sq_win.md
python tools/seq_probe.py > $D/${R}_seq_probe.txt 2>&1
python tools/win_probe.py > $D/${R}_win_probe.txt 2>&1
python tools/convergence_run.py 400 > $D/${R}_convergence_cfg2.txt 2>&1
python bench.py --full > $D/${R}_bench_default.json 2> $D/bench.err
tail -c 600 $D/${R}_bench_default.json
# gpurun merges at most 64 MiB back: the rocpd databases stay on the box
rm -rf gpurun_out/prof_${R} gpurun_out/prof_${R}_cfg4 gpurun_out/prof_${R}_cfg5 gpurun_out/sq_seq gpurun_out/sq_win
ls $D; du -sh gpurun_out
