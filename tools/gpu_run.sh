#!/bin/bash
# Staged GPU session for gpurun: every GPU step has its own time limit; a
# crash, abort or time-out (exit >= 124, or 134/139) ends the session, plain
# test failures (exit 1) do not.
#   tools/gpu_run.sh "<stage> <stage> ..."   stages: smoke tests bench prof loop
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}" || exit 2
R=$PWD; O=$(realpath -m "${OMG_OUT:-measurements}"); mkdir -p "$O"   # every stage's log
export TMPDIR=/tmp
STAGES="${1:-smoke tests bench prof}"
rc_ok() { [ "$1" -eq 0 ] || [ "$1" -eq 1 ]; }
for s in $STAGES; do
  echo "=== stage $s $(date +%T)"
  case $s in
    smoke) timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > "$O/smoke.log" 2>&1; rc=$? ;;
    tests) timeout -k 10 900 python -m pytest tests -m gpu -x -q ${PYTEST_ARGS:-} > "$O/pytest_gpu.log" 2>&1; rc=$? ;;
    bench) timeout -k 10 600 python bench.py --full ${BENCH_ARGS:-} > "$O/bench.log" 2>&1; rc=$? ;;
    prof) (cd /tmp && timeout -k 10 600 rocprofv3 --kernel-trace --stats -d "$O/prof" -o run --output-format csv -- python3 "$R/bench.py" --steps 5 --warmup 1 --full --no-cpu-baseline) > "$O/prof.log" 2>&1; rc=$? ;;
    loop) { timeout -k 10 300 python tools/loopback_bench.py 8 128 5 0 && timeout -k 10 300 python tools/loopback_bench.py 8 128 5 && \
            timeout -k 10 300 python tools/loopback_bench.py 2 256 5 0 && timeout -k 10 300 python tools/loopback_bench.py 2 256 5; } > "$O/loop.log" 2>&1; rc=$? ;;
    *) echo "unknown stage $s"; rc=2 ;;
  esac
  echo "=== stage $s rc=$rc $(date +%T)"
  tail -5 "$O"/$s*.log 2>/dev/null
  if ! rc_ok $rc; then echo "stopping after $s (rc=$rc)"; exit $rc; fi
done
exit 0
