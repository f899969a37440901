#!/bin/bash
# timeline of C5 queries: kernel + memory-copy trace (no counters)
set -o pipefail
cd "$GRAFT_REPO_ROOT"
export TMPDIR=/tmp FRS_BENCH_TMP=/dev/shm
R=$PWD O=${FRS_OUT:-$PWD/bench_out}/c5trace
mkdir -p $O
cd /tmp
timeout -k 10 300 rocprofv3 --kernel-trace --memory-copy-trace --hip-runtime-trace --output-format csv -d $O/raw -o run -- python3 $R/bench.py --full --no-extras --no-cpu --steps 1 --warmup 1 --queries 60 > $O/b.json 2> $O/b.err || { tail -20 $O/b.err; exit 1; }
cd $R
find $O/raw -name "*.csv" | head
