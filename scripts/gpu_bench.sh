set -o pipefail
O=${OUT:-bench_out}
mkdir -p $O
export TMPDIR=/tmp
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $O/smoke.log 2>&1 && \
DG_BENCH_DETAIL=1 timeout -k 10 600 python bench.py --full --steps 20 --warmup 6 --cpu-steps 3 > $O/bench.json 2> $O/bench.err && \
timeout -k 10 600 rocprofv3 --kernel-trace --stats -d $O/prof -o run --output-format csv -- python3 bench.py --profile-only --steps 5 --warmup 3 > $O/prof.log 2>&1
echo rc=$?
