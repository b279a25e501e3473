#!/bin/bash
# parent build vs new build, alternating, same box: 4 pairs of the headline and of the 20-step form
set -o pipefail
cd "$(dirname "$0")/.."
O=out/pipe; mkdir -p $O
export HEAT2D_PLAN_CACHE=off
PARENT=$PWD/jobs/parent/libheat2d.so
[ -f $PARENT ] || { echo "no parent library"; exit 2; }
one() {  # tag lib name args...
  local tag=$1 lib=$2 name=$3; shift 3
  if [ $lib = new ]; then unset HEAT2D_LIB; else export HEAT2D_LIB=$PARENT; fi
  timeout -k 10 300 python bench.py "$@" > $O/${name}_${tag}.json 2> $O/${name}_${tag}.err
  local rc=$?
  echo "$name $tag rc=$rc $(tail -1 $O/${name}_${tag}.json | cut -c1-110)"
  return $rc
}
for i in 1 2 3 4; do
  one parent_$i parent head || exit 1
  one new_$i new head || exit 1
  one parent_$i parent s20 --steps 20 --warmup 5 || exit 1
  one new_$i new s20 --steps 20 --warmup 5 || exit 1
done
