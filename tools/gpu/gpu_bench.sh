#!/bin/bash
# Default bench line (N = 1, all extras) -> $O/
set -o pipefail
cd "$GRAFT_REPO_ROOT"
export TMPDIR=/tmp FRS_BENCH_TMP=/dev/shm
O=${FRS_OUT:-$PWD/bench_out}/bench
mkdir -p $O
timeout -k 10 600 python -u bench.py --full ${BENCH_ARGS:-} > $O/bench.json 2> $O/bench.err || { tail -30 $O/bench.err; exit 1; }
cat $O/bench.json
