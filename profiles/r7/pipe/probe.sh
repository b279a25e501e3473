#!/bin/bash
# pair-pipeline probe: variants a (publish at the top of the row) and b (late publish)
set -o pipefail
cd "$(dirname "$0")/.."
O=out/pipe
mkdir -p $O
run() {  # variant n K
  local f=$O/probe_$1_$2_k$3
  timeout -k 10 120 jobs/bin/pipe_probe_$1 $2 $3 > $f.json 2> $f.err
  local rc=$?
  echo "variant $1 n=$2 K=$3 rc=$rc"; tail -5 $f.json; cat $f.err
  return $rc
}
run a 32768 20 && run b 32768 20 && run a 16384 20 && run a 32768 24 && run a 16384 24
