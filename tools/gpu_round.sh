#!/bin/bash
# Round evidence: GPU parity suite, the bench line with every leg (--full by
# VMP_BENCH_FULL, with the CPU baseline), then the rocprofv3 kernel-trace + PMC
# passes (tools/gpu_profile.sh, which switches the other legs off itself).
cd "$GRAFT_REPO_ROOT" || exit 1
mkdir -p gpurun_out
timeout -k 10 600 python -u -m pytest tests -x -v -m gpu --timeout 120 --timeout-method thread > gpurun_out/gpu_tests.log 2>&1
rc=$?; echo "tests_rc=$rc"; tail -3 gpurun_out/gpu_tests.log
[ $rc -ne 0 ] && exit $rc
export VMP_BENCH_FULL=1
timeout -k 10 400 python bench.py > gpurun_out/bench.log 2>&1
rc=$?; echo "bench_rc=$rc"; tail -1 gpurun_out/bench.log
[ $rc -ne 0 ] && exit $rc
bash tools/gpu_profile.sh
