# One GPU round trip: parity tests, full bench (no CPU legs), kernel-trace profile.
# Results go to $O (default: out/ under the repository root).
export TMPDIR=/tmp
O=${O:-out}
mkdir -p $O
timeout -k 10 300 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread > $O/pytest_gpu.log 2>&1
echo "pytest rc=$?" >> $O/pytest_gpu.log
tail -3 $O/pytest_gpu.log
grep -q "pytest rc=0" $O/pytest_gpu.log || exit 1
timeout -k 10 300 python -u bench.py --full --steps 20 --warmup 3 --no-cpu ${BENCH_ARGS} > $O/bench.json 2> $O/bench.err || exit 2
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $O/prof2 -o run --output-format csv -- python bench.py --full --steps 10 --warmup 2 --no-cpu --games 2000000 ${BENCH_ARGS} > /dev/null 2> $O/prof.err || exit 3
cat $O/bench.json
