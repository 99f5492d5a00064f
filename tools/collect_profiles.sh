# Collects the per-round evidence on the GPU box: bench line, kernel-trace summary, the two PMC traffic passes, the MFMA
# utilisation pass and the per-shape table.  usage: bash tools/collect_profiles.sh [out_dir]   (default build/profiles;
# then copy <out_dir>/* to profiles/)
set -e
export TMPDIR=/tmp
cd "$(dirname "$0")/.."
G="${1:-build/profiles}"
mkdir -p "$G"
# the profiled command is the HEADLINE workload's canonical steps and nothing else (DEPGAN_BENCH_STEP_ONLY: no
# generator-forward / generator-iteration probes, no extra engines): per-kernel averages and PMC sums then cover exactly
# the launches bench.py's `roofline` describes, and the class launch count is steps x launches-per-step
export DEPGAN_BENCH_STEP_ONLY=1
DEPGAN_PROFILE_DUMP="$G/launches.csv" python bench.py --full --steps 5 --warmup 2 --no-cpu-baseline > "$G/bench_short.json" 2> "$G/bench.err"
python3 tools/layer_table.py "$G/launches.csv" 2 > "$G/layer_table.md"
echo dump done
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d "$G/kt" -o r --output-format csv -- python3 bench.py --full --steps 5 --warmup 2 --no-cpu-baseline > "$G/kt.log" 2>&1
echo kt done
timeout -k 10 300 rocprofv3 --pmc FETCH_SIZE --kernel-trace -d "$G/pf" -o r --output-format csv -- python3 bench.py --full --steps 2 --warmup 1 --no-cpu-baseline > "$G/pf.log" 2>&1
echo pf done
timeout -k 10 300 rocprofv3 --pmc WRITE_SIZE --kernel-trace -d "$G/pw" -o r --output-format csv -- python3 bench.py --full --steps 2 --warmup 1 --no-cpu-baseline > "$G/pw.log" 2>&1
echo pw done
timeout -k 10 300 rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE --kernel-trace -d "$G/mu" -o r --output-format csv -- python3 bench.py --full --steps 2 --warmup 1 --no-cpu-baseline > "$G/mu.log" 2>&1
echo mu done
python3 tools/pmc_traffic.py "$G/pf" "$G/pw" "$G/pmc_traffic.json"
python3 tools/pmc_mfma_util.py "$G/mu" "$G/mfma_util.json"
cp $(find "$G/kt" -name "*kernel_stats.csv" | head -1) "$G/kernel_stats.csv"
rm -rf "$G/kt" "$G/pf" "$G/pw" "$G/mu"
unset DEPGAN_BENCH_STEP_ONLY
python bench.py --full > "$G/bench.json" 2>> "$G/bench.err"
echo bench done
tail -c 600 "$G/bench.json"
