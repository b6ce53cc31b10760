#!/bin/bash
# One GPU call: gpu parity tests, default bench (with CPU baseline), C4/C5 benches, round profile.
# Usage: tools/gpu_session.sh rNN   (each step time-limited; stops at the first failure)
set -o pipefail
R=${1:-r01}
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
RESULTS=${RESULTS:-bench_results}
mkdir -p $RESULTS
timeout -k 10 900 python -u -m pytest tests -m gpu -x -q -ra --timeout 300 --timeout-method thread > $RESULTS/tests_$R.log 2>&1 && \
timeout -k 10 600 python bench.py --full > $RESULTS/bench_$R.json 2> $RESULTS/bench_$R.err && \
timeout -k 10 300 python bench_mll.py > $RESULTS/bench_mll_$R.json 2> $RESULTS/bench_mll_$R.err && \
timeout -k 10 300 python bench_split.py > $RESULTS/bench_split_$R.json 2> $RESULTS/bench_split_$R.err && \
bash tools/profile_round.sh $R
rc=$?
echo "session rc=$rc"
tail -3 $RESULTS/tests_$R.log; cat $RESULTS/bench_$R.json
exit $rc
