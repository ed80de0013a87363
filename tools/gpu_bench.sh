# One GPU call: rocprofv3 kernel stats, two PMC passes (HBM bytes), then the full bench line.
# Run from anywhere; results go to $OUT (default profile_out/ in the repository root).
set -o pipefail
cd "$(dirname "$0")/.."
TAG=${TAG:-r01}
OUT=${OUT:-profile_out}
mkdir -p "$OUT"
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/${TAG}_stats" -o run -- python3 bench.py --full --steps 5 --warmup 2 --no-cpu > "$OUT/${TAG}_stats.log" 2>&1 && \
timeout -k 10 600 rocprofv3 --pmc FETCH_SIZE --output-format csv -d "$OUT/${TAG}_pmc_fetch" -o run -- python3 bench.py --full --steps 2 --warmup 1 --no-cpu > "$OUT/${TAG}_pmc_fetch.log" 2>&1 && \
timeout -k 10 600 rocprofv3 --pmc WRITE_SIZE --output-format csv -d "$OUT/${TAG}_pmc_write" -o run -- python3 bench.py --full --steps 2 --warmup 1 --no-cpu > "$OUT/${TAG}_pmc_write.log" 2>&1 && \
sha256sum sgufp_solver_amd/lib/libsgufp_hip.so | cut -d' ' -f1 > "$OUT/${TAG}_pmc_fetch/lib.sha256" && \
cp "$OUT/${TAG}_pmc_fetch/lib.sha256" "$OUT/${TAG}_pmc_write/lib.sha256" && \
echo "C4:seed1:nodes8192:pool16F+64O" > "$OUT/${TAG}_pmc_fetch/workload.txt" && \
cp "$OUT/${TAG}_pmc_fetch/workload.txt" "$OUT/${TAG}_pmc_write/workload.txt" && \
mkdir -p profiles && cp -r "$OUT/${TAG}_pmc_fetch" "$OUT/${TAG}_pmc_write" profiles/ && \
timeout -k 10 600 python3 bench.py --full --profile-tag ${TAG} > "$OUT/bench_${TAG}.json" 2> "$OUT/bench_${TAG}.err"
