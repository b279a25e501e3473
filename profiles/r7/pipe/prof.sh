#!/bin/bash
# before / after records: kernel trace, counters (a run of their own), --measure-hbm, --full
set -o pipefail
cd "$(dirname "$0")/.."
O=$PWD/out/pipe; mkdir -p $O
export HEAT2D_PLAN_CACHE=off
PARENT=$PWD/jobs/parent/libheat2d.so
for lib in parent new; do
  if [ $lib = new ]; then unset HEAT2D_LIB; else export HEAT2D_LIB=$PARENT; fi
  timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O/trace_$lib -o t -- python bench.py --steps 20 --warmup 5 > $O/trace_$lib.json 2> $O/trace_$lib.err
  rc=$?; echo "trace $lib rc=$rc"; [ $rc -eq 0 ] || exit $rc
  timeout -k 10 400 rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_LDS SQ_WAVE_CYCLES SQ_WAIT_INST_ANY SQ_BUSY_CYCLES GRBM_GUI_ACTIVE --output-format csv -d $O/pmc_$lib -o c -- python bench.py --steps 20 --warmup 5 > $O/pmc_$lib.json 2> $O/pmc_$lib.err
  rc=$?; echo "pmc $lib rc=$rc"; [ $rc -eq 0 ] || exit $rc
  timeout -k 10 400 python bench.py --steps 20 --warmup 5 --measure-hbm > $O/hbm_$lib.json 2> $O/hbm_$lib.err
  rc=$?; echo "hbm $lib rc=$rc"; [ $rc -eq 0 ] || exit $rc
done
unset HEAT2D_LIB
timeout -k 10 400 python bench.py --full > $O/full_new.json 2> $O/full_new.err
rc=$?; echo "full rc=$rc"; tail -1 $O/full_new.json | cut -c1-300
# shrink what comes back: per-kernel stats and summed counters only
python3 jobs/summarize.py $O > $O/prof_summary.json; cat $O/prof_summary.json | head -80
find $O -name "*kernel_trace.csv" -delete; find $O -name "*counter_collection.csv" -delete
exit $rc
