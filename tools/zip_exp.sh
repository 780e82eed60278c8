#!/bin/bash
# Development: parity + quick headline bench of k_zip_f32 experiment builds (make EXP=n), stamps of the STAMPS builds;
# outputs in $OUT (default bench_out/):
#   bash tools/zip_exp.sh "0 1 2 3" "8 9 10 11"
set -o pipefail
OUT=${OUT:-bench_out}; mkdir -p "$OUT"
for e in $1; do
  lib=contractn_amd/lib/libctn_hip_exp$e.so; [ $e = 0 ] && lib=contractn_amd/lib/libctn_hip.so
  CTN_LIB_PATH=$PWD/$lib timeout -k 10 200 python -m pytest tests/test_gpu_parity.py -q -k zip > "$OUT/zexp_t$e.log" 2>&1 || { echo "exp $e: tests FAILED"; tail -5 "$OUT/zexp_t$e.log"; continue; }
  CTN_LIB_PATH=$PWD/$lib timeout -k 10 200 python bench.py --full --no-peps --no-batched --no-cpu-baseline --no-latency --steps 6 > "$OUT/zexp_b$e.json" 2> "$OUT/zexp_b$e.err" || { echo "exp $e: bench FAILED"; exit 1; }
  python - <<PY
import json
d=json.loads(open("$OUT/zexp_b$e.json").read().strip().splitlines()[-1])
print("exp $e", d["value"], d["roofline"]["frac"], d["roofline"]["avg_launch_us"])
PY
done
for e in $2; do
  CTN_LIB_PATH=$PWD/contractn_amd/lib/libctn_hip_exp$e.so timeout -k 10 200 python tools/stamps_zip.py 512 > "$OUT/zexp_s$e.log" 2>&1; echo "stamps $e: $(tail -1 "$OUT/zexp_s$e.log")"
done
