#!/bin/bash
# One GPU-box visit: gpu tests, smoke, bench, rocprofv3 kernel trace + PMC passes.  usage: gpu_round.sh TAG [OUT_DIR]
# Outputs under OUT_DIR (default build/gpu_round/<TAG>).
TAG=${1:-r01}; O=${2:-build/gpu_round/$TAG}
mkdir -p $O
timeout 900 python3 -m pytest tests -m gpu -x -q -s > $O/pytest_gpu.log 2>&1; echo "pytest rc=$?" >> $O/pytest_gpu.log
timeout 300 python3 -c "import __graft_entry__ as g; g.smoke()" > $O/smoke.log 2>&1; echo "smoke rc=$?" >> $O/smoke.log
timeout 600 python3 bench.py --full > $O/bench_$TAG.log 2>&1; echo "bench rc=$?" >> $O/bench_$TAG.log
export TMPDIR=/tmp
rm -rf $O/prof_kt
timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_kt -- python3 bench.py --full --steps 50 --warmup 10 --no-cpu-baseline > $O/prof_kt.log 2>&1; echo "rocprof rc=$?" >> $O/prof_kt.log
PMC_OUT=$O/pmc bash scripts/gpu_pmc.sh > $O/pmc.log 2>&1
tail -4 $O/pytest_gpu.log; tail -2 $O/smoke.log; tail -2 $O/bench_$TAG.log | cut -c1-900
