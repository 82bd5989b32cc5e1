#!/bin/bash
# configs[4]'s k = 12 slice: per-tier item counts (SA_DEBUG_TIERS) and rocprofv3
# kernel stats, packed tier ($1 = 1) or the two-word table ($1 = 0).
set -u
R=$PWD
O=${SA_PROF_OUT:-$R/prof_out}
mkdir -p $O
cd /tmp && export TMPDIR=/tmp
export SA_DEBUG_TIERS=1 SA_PACKED_TIER=$1
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $O/c4p$1 -o run -- python3 $R/bench.py --full --no-cpu-baseline --reads 6250000 --len 1000 --min-len 100 --k 12 --steps 1 --warmup 0 --align-steps 1 > $O/c4p$1.log 2>&1
echo "c4p$1 rc=$?" >> $O/steps.txt
