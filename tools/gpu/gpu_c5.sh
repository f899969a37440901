#!/bin/bash
# C5 path: pipe-decoder parity, then the C4 step + 1000 bbox queries (twice)
set -o pipefail
cd "$GRAFT_REPO_ROOT"
export TMPDIR=/tmp FRS_BENCH_TMP=/dev/shm
O=${FRS_OUT:-$PWD/bench_out}/c5
mkdir -p $O
timeout -k 10 600 python -u -m pytest ${C5_TESTS:-tests/test_gpu_decode.py tests/test_gpu_configs.py} -x -v --timeout 120 --timeout-method thread > $O/tests.log 2>&1 || { tail -60 $O/tests.log; exit 1; }
tail -2 $O/tests.log
for r in 1 2; do
timeout -k 10 300 python -u bench.py --full --no-extras --no-cpu --steps 5 --queries 1000 > $O/b$r.json 2> $O/b$r.err || { tail -30 $O/b$r.err; exit 1; }
python -c "
import json; d=json.load(open('$O/b$r.json')); b=d['bbox_extract']
print('step', d['ms_per_step'], 'p50', b['p50_ms'], 'p90', b['p90_ms'], b['kernels_ms_rank0'])"
done
