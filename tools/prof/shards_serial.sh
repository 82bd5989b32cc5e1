#!/bin/bash
# Kernel stats of 8 virtual shards run one after another (SA_OPT_SERIAL_SHARDS):
# per-shard stage times for DESIGN.md 7 (profiles/<round>/sharded/).
set -u
R=$PWD
O=${SA_PROF_OUT:-$R/prof_out}
mkdir -p $O
cd /tmp && export TMPDIR=/tmp
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O/p_sh -o run -- python3 $R/bench.py --full --shards 8 --serial-shards --steps 3 --warmup 1 --no-cpu-baseline --align-steps 1 > $O/p_sh.log 2>&1 || exit 1
