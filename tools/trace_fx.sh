#!/bin/bash
# kernel trace + SQ counters of the fixed-point leg (bench.py --full legs, the fixed-point kernels picked out); output under
# $PROFILE_OUT (default: profile_out/ in the repository)
R=${GRAFT_REPO_ROOT:-$PWD}; cd /tmp; export TMPDIR=/tmp
O=${PROFILE_OUT:-$R/profile_out}; mkdir -p $O
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O/tr_fx -- python3 $R/bench.py --steps 10 --warmup 2 --full --no-cpu > $O/tr_fx.log 2>&1 &&
timeout -k 10 300 rocprofv3 --pmc SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_INSTS_LDS SQ_WAIT_INST_ANY SQ_INSTS_SALU SQ_WAVES --output-format csv -d $O/pm_fx -- python3 $R/bench.py --steps 4 --warmup 2 --full --no-cpu > $O/pm_fx.log 2>&1
grep "sk_fx" $O/tr_fx/*/*kernel_stats.csv
