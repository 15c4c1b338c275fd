export TMPDIR=/tmp
for v in 0 3; do
  OUT=gpurun_out/kt_ps$v; rm -rf $OUT; mkdir -p $OUT
  LAV_GEMM_PS=$v rocprofv3 --kernel-trace --stats -d $OUT/kt -o kt -- python bench.py --steps 10 --warmup 3 --full --no-cpu-baseline --no-ref-loop > $OUT/kt.log 2>&1
  KT=$(find $OUT/kt -name "*_results.db" | head -1)
  python tools/rocpd_stats.py $KT gpurun_out/kt_ps$v.md > /dev/null
  python tools/timeline.py $KT gpurun_out/tl_ps$v.md > /dev/null 2>&1
  grep -h '^{"metric"' $OUT/kt.log | python -c "import sys,json; d=json.loads(sys.stdin.read()); print('PS=$v', d['ms_per_step'])"
  rm -rf $OUT
done
