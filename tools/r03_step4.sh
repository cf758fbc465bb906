#!/bin/bash
set -o pipefail
root=$(cd "$(dirname "$0")/.." && pwd)
out=$root/${1:-profile_out}
mkdir -p $out
timeout -k 10 1100 python -m pytest tests/test_fullsize_properties_gpu.py tests/test_parity_gpu.py -x -q > $out/r03_step4_tests.log 2>&1
echo "tests rc=$?"; tail -3 $out/r03_step4_tests.log
for pct in 45 30 60; do
python - <<PY
import json, subprocess, sys
PY
done
timeout -k 10 600 python bench.py --full --len 500 --width 30 --order 4 --steps 12 --warmup 12 --no-cpu-baseline 2>>$out/r03_step4_bench.err | tee $out/r03_step4_c4.json | python -c "
import sys,json
for l in sys.stdin:
    j=json.loads(l); print('C4 ms_per_step', round(j['ms_per_step'],4), 'cold', j.get('ms_per_step_cold'), 'opt', j.get('ms_per_step_optimize_mode'))"
cd /tmp && export TMPDIR=/tmp && rocprofv3 --kernel-trace --stats -d $out/r03_c4_prof -o c4 -- python3 $root/bench.py --full --len 500 --width 30 --order 4 --steps 0 --warmup 0 --no-cpu-baseline > /dev/null 2>>$out/r03_step4_bench.err; cd $root
find $out/r03_c4_prof -name "*kernel_stats*" | head -3
