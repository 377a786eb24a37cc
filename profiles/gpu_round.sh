#!/bin/bash
# One GPU call: the -m gpu suite (no -x: every failure is listed), then -- unless the suite
# ended on a fault, abort or time limit -- the full bench (bench.py --full).
# Usage: gpu_round.sh OUTDIR TAG [pytest args]
out=${1:?output directory}; tag=${2:?tag}; shift 2
mkdir -p "$out"
timeout -k 10 900 python -u -m pytest tests -m gpu -v --timeout 600 --timeout-method thread "$@" \
  > "$out/gputest_$tag.log" 2>&1
rc=$?
echo "pytest rc=$rc"
tail -30 "$out/gputest_$tag.log"
if [ $rc -ne 0 ] && [ $rc -ne 1 ]; then exit $rc; fi
timeout -k 10 600 python -u bench.py --full > "$out/bench_$tag.json" 2> "$out/bench_$tag.err"
brc=$?
echo "bench rc=$brc"
tail -c 3000 "$out/bench_$tag.json"
exit $brc
