#!/bin/bash
# Round 6: the default bench line (as the driver runs it), then tools/prof/profile.sh
# (kernel stats + PMC passes of the default workload).
set -u
P=${SA_PROF_OUT:-prof_out}
mkdir -p $P/r6fin
timeout -k 10 600 python bench.py --full > $P/r6fin/bench_default.log 2>&1 || exit 1
tail -1 $P/r6fin/bench_default.log > $P/r6fin/bench_default.json
python3 -c 'import json,sys; d=json.load(open(sys.argv[1])); print(d["ms_per_step"], d["value"], d["ms_per_align_step"], d["roofline"]["frac"], d["config0"]["gpu_end_to_end_s"], d["config2_end_to_end"]["total_s"])' $P/r6fin/bench_default.json
rm -rf $P/prof $P/pmc_*
bash tools/prof/profile.sh > $P/r6fin/profile.log 2>&1 || exit 1
tail -3 $P/steps.txt
