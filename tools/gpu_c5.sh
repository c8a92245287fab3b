#!/bin/bash
# The C4 / C5 config tests, then a full C5 (llama7b) bench line with its kernel averages.
# Logs go to $OUT_DIR (default bench_out/).
cd "$(dirname "$0")/.." || exit 1
out=${OUT_DIR:-bench_out}
mkdir -p "$out"
timeout -k 10 600 python -u -m pytest tests/test_gpu_configs.py tests/test_gpu_reference.py -x -q -rf --timeout 300 --timeout-method thread > "$out/cfg_tests.log" 2>&1; rc=$?; tail -3 "$out/cfg_tests.log"; [ $rc -eq 0 ] || exit $rc
timeout -k 10 600 python -u bench.py --full --model llama7b --steps 2 --warmup 1 --no-cpu-baseline > "$out/bench_llama_w.log" 2>&1 || exit $?
python -c "
import json, sys; d=json.loads([l for l in open(sys.argv[1]) if l.startswith('{')][-1]); print(round(d['value']), round(d['ms_per_step'],1), {k: round(v,1) for k,v in d['kernel_avg_us'].items()})" "$out/bench_llama_w.log"
