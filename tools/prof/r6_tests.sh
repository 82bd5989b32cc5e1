#!/bin/bash
# Round 6: a GPU test subset (TESTS, -k filter K) into $P/$OUT/tests.log.
set -u
P=${SA_PROF_OUT:-prof_out}
OUT=${OUT:-r6}
mkdir -p $P/$OUT
timeout -k 10 ${SECS:-900} python -u -m pytest ${TESTS:-tests/test_gpu_sharded.py} -m gpu -x -v \
    --timeout ${PER:-400} --timeout-method thread ${EXTRA:-} ${K:+-k "$K"} > $P/$OUT/tests.log 2>&1
rc=$?
tail -5 $P/$OUT/tests.log
exit $rc
