#!/bin/bash
# sharded parity tests, then same-box per-shard A/B (tools/prof/shard_ab.sh)
set -u
P=${SA_PROF_OUT:-prof_out}
mkdir -p $P/shard_ab
timeout -k 10 600 python -u -m pytest ${TESTS:-tests/test_gpu_sharded.py} -m gpu -x -q --timeout 300 --timeout-method thread > $P/shard_ab/tests.log 2>&1
rc=$?; tail -3 $P/shard_ab/tests.log; [ $rc -eq 0 ] || exit $rc
rm -f $P/shard_ab/ab.txt
VARIANTS="${VARIANTS:-build_base build}" REPS=${REPS:-2} bash tools/prof/shard_ab.sh
