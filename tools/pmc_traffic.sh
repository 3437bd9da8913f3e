#!/bin/bash
# HBM-side traffic of the bench workload: two separate rocprofv3 PMC passes (never combined with other trace domains).
# usage (needs the GPU): bash tools/pmc_traffic.sh   -> prof_out/hbm_traffic.{txt,json}
R=$(cd "$(dirname "$0")/.." && pwd)
O=${AMS_PROF_OUT:-$R/prof_out}          # outputs: prof_out/ in the tree unless AMS_PROF_OUT names another folder
mkdir -p $O
export AMS_COMMIT=${AMS_COMMIT:-$(cat $R/.ams_commit 2>/dev/null || echo unknown)}
cd /tmp && export TMPDIR=/tmp
CMD="python $R/bench.py --full --no-cpu-baseline --no-secondary --no-native-f32 --graph 0 --steps 3 --warmup 2 --roofline-steps 1 --quiet"
for C in FETCH_SIZE WRITE_SIZE; do
  rm -rf /tmp/pmc_$C
  timeout 900 rocprofv3 --pmc $C --kernel-trace -d /tmp/pmc_$C -o run -- $CMD > $O/pmc_$C.log 2>&1
done
F=$(find /tmp/pmc_FETCH_SIZE -name "*.db" | head -1); W=$(find /tmp/pmc_WRITE_SIZE -name "*.db" | head -1)
python $R/tools/pmc_summary.py $F $W $O/hbm_traffic.txt $O/hbm_traffic.json "bench.py --full --no-cpu-baseline --no-secondary --no-native-f32 --graph 0 --steps 3 --warmup 2 --roofline-steps 1"
