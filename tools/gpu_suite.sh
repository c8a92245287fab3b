#!/bin/bash
# One GPU session: the GPU test suite (or the given pytest selection), then - only if
# it ended without a fault, abort or timeout - a full bench line (`bench.py --full`).
# Outputs under $OUT_DIR/<tag>_* (default bench_out/). Usage: tools/gpu_suite.sh TAG [pytest-args...]
cd "$(dirname "$0")/.." || exit 1
tag=${1:-run}; shift
out=${OUT_DIR:-bench_out}
mkdir -p "$out"
sel=("$@"); [ ${#sel[@]} -eq 0 ] && sel=(tests -m gpu)
timeout -k 10 1100 python -u -m pytest "${sel[@]}" -x -q -rf --timeout 300 --timeout-method thread \
  > "$out/${tag}_pytest.log" 2>&1
rc=$?
echo "pytest rc=$rc"; tail -15 "$out/${tag}_pytest.log"
[ $rc -ne 0 ] && exit $rc
timeout -k 10 300 python -u bench.py --full --steps 10 --warmup 2 > "$out/${tag}_bench.json" 2> "$out/${tag}_bench.err"
brc=$?
echo "bench rc=$brc"; tail -c 1500 "$out/${tag}_bench.json"
exit $brc
