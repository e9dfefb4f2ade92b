#!/bin/bash
# One measurement pass on the GPU box: headline bench, configs 4/5, encoder kernel trace,
# bench kernel trace and the FETCH/WRITE PMC passes for profiles/.  Results go to $OUT
# (default measure_out/ under the repo root).  The bench runs take --full: the records
# hold the latency, roofline, config-2 and CPU-baseline passes beside the headline.
set -e
cd "$(dirname "$0")/.."
OUT=${OUT:-measure_out}
mkdir -p "$OUT"
timeout -k 10 600 python bench.py --full > "$OUT/bench.json" 2> "$OUT/bench.err"
timeout -k 10 400 python bench.py --full --arch res18trans --no-cpu-baseline > "$OUT/bench_res18.json" 2>> "$OUT/bench.err"
timeout -k 10 600 python bench.py --full --beam 4 --batch 32 --tokens 256 --steps 6 --warmup 2 --no-cpu-baseline > "$OUT/bench_beam.json" 2>> "$OUT/bench.err"
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof_bench" -o run -- \
  python3 bench.py --full --steps 4 --warmup 1 --no-cpu-baseline > "$OUT/prof_bench.log" 2>&1
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof_enc" -o run -- python3 tools/profile_encoder.py --encodes 3 > "$OUT/prof_enc.log" 2>&1
timeout -k 10 300 rocprofv3 --pmc FETCH_SIZE --output-format csv -d "$OUT/pmc_f" -o run -- python3 tools/profile_encoder.py > "$OUT/pmc_f.log" 2>&1
timeout -k 10 300 rocprofv3 --pmc WRITE_SIZE --output-format csv -d "$OUT/pmc_w" -o run -- python3 tools/profile_encoder.py > "$OUT/pmc_w.log" 2>&1
echo done
