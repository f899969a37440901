#!/bin/bash
# kernel stats of a whole bench run (all legs)
set -o pipefail
cd "$GRAFT_REPO_ROOT"
export TMPDIR=/tmp FRS_BENCH_TMP=/dev/shm
R=$PWD O=${FRS_OUT:-$PWD/bench_out}/profall
mkdir -p $O
cd /tmp
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $O/raw -o run -- python3 $R/bench.py --full --no-cpu --queries 200 --steps 5 > $O/bench.json 2> $O/bench.err || { tail -20 $O/bench.err; exit 1; }
cd $R
f=$(find $O/raw -name "*kernel_stats.csv" | head -1)
cp "$f" $O/kernel_stats.csv
python3 - <<PY
import csv
rows=list(csv.DictReader(open('$O/kernel_stats.csv')))
rows.sort(key=lambda r: -float(r['TotalDurationNs']))
for r in rows[:40]:
    print(f"{r['Name'][:90]:90s} n={r['Calls']:>6s} avg={float(r['AverageNs'])/1e3:9.1f}us tot={float(r['TotalDurationNs'])/1e6:8.2f}ms")
PY
