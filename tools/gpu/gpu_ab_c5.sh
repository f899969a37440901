#!/bin/bash
set -o pipefail
cd "$GRAFT_REPO_ROOT"
export TMPDIR=/tmp
O=${FRS_OUT:-$PWD/bench_out}/c5
mkdir -p $O
for a in "--steps 5 --warmup 2" "--steps 10 --warmup 5" "--steps 5 --warmup 2"; do
  timeout -k 10 300 python -u bench.py --full $a --no-extras --no-cpu > $O/run.json 2> $O/run.err || { tail -20 $O/run.err; exit 1; }
  python -c "import json;d=json.load(open('$O/run.json'));print('$a', d['ms_per_step'], d['bbox_extract']['p50_ms'], d['bbox_extract']['p90_ms'])"
done
