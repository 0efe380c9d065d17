#!/bin/bash
# rocprofv3 evidence for the bench line: kernel-trace stats of the bench command itself, then FETCH_SIZE and
# WRITE_SIZE passes (separate runs, counters only), and a FETCH_SIZE pass on the dense query (every row read)
# to calibrate the counter for this kernel's access widths. Summary -> $OUT/pmc_<query>.json.
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
OUT=${OUT:-bench_out}   # where the outputs go (git-ignored)
mkdir -p $OUT/prof
export TMPDIR=/tmp
Q=${QUERY:-c2}
rm -rf $OUT/prof/bench_kt $OUT/prof/bench_fetch $OUT/prof/bench_write $OUT/prof/dense_fetch
timeout -k 10 600 rocprofv3 --kernel-trace --stats -d $OUT/prof/bench_kt -o kt --output-format csv -- python3 bench.py --full --query $Q --steps 10 --warmup 3 --cpu-sample 0 > $OUT/prof/bench_kt.json 2> $OUT/prof/bench_kt.log || exit $?
timeout -k 10 600 rocprofv3 --pmc FETCH_SIZE -d $OUT/prof/bench_fetch -o pmc --output-format csv -- python3 bench.py --full --query $Q --steps 3 --warmup 1 --cpu-sample 0 > $OUT/prof/bench_fetch.json 2> $OUT/prof/bench_fetch.log || exit $?
timeout -k 10 600 rocprofv3 --pmc WRITE_SIZE -d $OUT/prof/bench_write -o pmc --output-format csv -- python3 bench.py --full --query $Q --steps 3 --warmup 1 --cpu-sample 0 > $OUT/prof/bench_write.json 2> $OUT/prof/bench_write.log || exit $?
if [ -z "$NODENSE" ]; then
  timeout -k 10 600 rocprofv3 --pmc FETCH_SIZE -d $OUT/prof/dense_fetch -o pmc --output-format csv -- python3 bench.py --full --query dense --steps 3 --warmup 1 --cpu-sample 0 > $OUT/prof/dense_fetch.json 2> $OUT/prof/dense_fetch.log || exit $?
fi
mkdir -p $OUT/prof_$Q && cp -r $OUT/prof/bench_* $OUT/prof_$Q/ && python3 scripts/pmc_traffic.py $OUT/prof $Q > $OUT/pmc_$Q.json && cat $OUT/pmc_$Q.json
