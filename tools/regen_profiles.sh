#!/bin/bash
# Regenerate the evidence under profiles/ on a GPU machine (run from the repo root; outputs go to $OUT, default bench_out/):
#   bash tools/regen_profiles.sh r03      then, on any machine,
#   python profiles/make_summary.py r03 bench_out/prof_r03 bench_out/pmc_fetch bench_out/pmc_write bench_out/pmc_sq bench_out/bench_default.json
#   cp bench_out/bench_default.json profiles/r03_bench.json; cp bench_out/bench_f64.json profiles/r03_bench_f64.json
# Counters are collected in their own passes (no trace domains next to --pmc); the program itself follows `--`.
# The bench runs use --full: the lines carry the roofline, the CPU baseline and the secondaries the summaries read.
set -o pipefail
tag=${1:-r03}
R=$(pwd)
mkdir -p "${OUT:-bench_out}" && OUT=$(cd "${OUT:-bench_out}" && pwd)
B="--full --no-cpu-baseline --no-peps"
run() { name=$1; secs=$2; shift 2; echo "== $name"; timeout -k 10 $secs "$@" > $OUT/$name.log 2>&1; rc=$?; echo "== $name rc=$rc"; [ $rc -ge 124 ] && exit $rc; return 0; }
timeout -k 10 500 python bench.py --full > $OUT/bench_default.json 2> $OUT/bench_default.err; echo "bench_default rc=$?"
timeout -k 10 300 python bench.py --full --dtype f64 --replicas 256 --cpu-seconds 5 --no-peps > $OUT/bench_f64.json 2> $OUT/bench_f64.err; echo "bench_f64 rc=$?"
cd /tmp && export TMPDIR=/tmp
run prof_$tag 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_$tag -- python3 $R/bench.py $B
run pmc_fetch 300 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $OUT/pmc_fetch -- python3 $R/bench.py --steps 2 --warmup 1 $B
run pmc_write 300 rocprofv3 --pmc WRITE_SIZE --output-format csv -d $OUT/pmc_write -- python3 $R/bench.py --steps 2 --warmup 1 $B
run pmc_sq 300 rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE --output-format csv -d $OUT/pmc_sq -- python3 $R/bench.py --steps 2 --warmup 1 $B
cd $R
# the secondary configs and the sliced 8 x 8 PEPS (copied to profiles/<tag>_config_bench.jsonl, <tag>_peps_D8_bench.json /
# _steps.json / _kernel_stats.csv, <tag>_peps_D16_bench.json / _steps.json / _kernel_stats.csv afterwards)
timeout -k 10 500 python tools/config_bench.py > $OUT/${tag}_config_bench.jsonl 2> $OUT/config_bench.err; echo "config_bench rc=$?"
timeout -k 10 300 python bench.py --full --config peps --bond 8 --steps 20 --warmup 3 --dump-steps $OUT/${tag}_peps_D8_steps.json > $OUT/${tag}_peps_D8_bench.json 2> $OUT/peps_D8.err; echo "peps D8 rc=$?"
timeout -k 10 500 python bench.py --full --config peps --bond 16 --max-intermediate 4294967296 --steps 1 --warmup 1 --cross-check --no-cpu-baseline --dump-steps $OUT/${tag}_peps_D16_steps.json > $OUT/${tag}_peps_D16_bench.json 2> $OUT/peps_D16.err; echo "peps D16 rc=$?"
cd /tmp
run prof_peps8 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_peps8 -- python3 $R/bench.py --config peps --bond 8 --steps 20 --warmup 3 --no-cpu-baseline
run prof_peps16 400 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_peps16 -- python3 $R/bench.py --config peps --bond 16 --max-intermediate 4294967296 --steps 1 --warmup 1 --no-cpu-baseline --event-passes 0
run pmc_sq_peps16 400 rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE --output-format csv -d $OUT/pmc_sq_peps16 -- python3 $R/bench.py --config peps --bond 16 --max-intermediate 4294967296 --steps 1 --warmup 1 --no-cpu-baseline --event-passes 0
cd $R
tail -1 $OUT/bench_default.json | cut -c1-300
