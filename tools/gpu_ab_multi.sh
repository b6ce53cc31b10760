#!/bin/bash
# Same-box comparison of several prebuilt libraries (GPR_HIP_LIB): DAG parity subset per
# library, then C3 rounds in rotation.  Usage: tools/gpu_ab_multi.sh reps lib1 lib2 ...
cd $(dirname "$0")/..
RESULTS=${RESULTS:-bench_results}
mkdir -p $RESULTS
out=$RESULTS/ab_multi.txt; : > $out
R=$1; shift
for lib in "$@"; do
  GPR_HIP_LIB=$PWD/$lib timeout -k 10 200 python -u -m pytest tests/test_gpu_parity.py -x -q -k "potrf_dag or fit_predict_dag" --timeout 60 --timeout-method thread > $RESULTS/abm_tests.log 2>&1 || { echo "$lib tests FAILED" >> $out; exit 1; }
  echo "$lib $(tail -1 $RESULTS/abm_tests.log)" >> $out
done
for r in $(seq $R); do
  for lib in "$@"; do
    GPR_HIP_LIB=$PWD/$lib timeout -k 10 200 python bench.py --full --no-cpu-baseline --no-split --steps 3 --warmup 1 > $RESULTS/abm.json 2>/dev/null || exit 1
    python3 -c "import json;d=json.load(open('$RESULTS/abm.json'));print('$lib C3', round(d['ms_per_step'],2), 'ms dag', round(d['dag_ms'],2))" >> $out
  done
done
