# Round profile set: the full bench line (with the CPU baseline), rocprofv3 kernel stats, and the two
# PMC traffic passes of the conv engine (FETCH_SIZE and WRITE_SIZE in separate runs).
set -o pipefail
O=${OUT:-bench_out}
mkdir -p $O
export TMPDIR=/tmp
timeout -k 10 600 python bench.py --full --steps 30 --warmup 8 > $O/bench.json 2> $O/bench.err && \
timeout -k 10 600 rocprofv3 --kernel-trace --stats -d $O/prof -o run --output-format csv -- python3 bench.py --profile-only --steps 10 --warmup 4 > $O/prof.log 2>&1 && \
bash scripts/gpu_pmc_bench.sh
