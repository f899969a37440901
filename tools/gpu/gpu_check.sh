#!/bin/bash
# Re-entry check: smoke, GPU parity suite, one default-size bench line (no CPU leg).
set -o pipefail
cd "$GRAFT_REPO_ROOT"
export TMPDIR=/tmp
O=${FRS_OUT:-$PWD/bench_out}/check
mkdir -p $O
timeout -k 10 300 python -u -c "import __graft_entry__ as g; g.smoke()" > $O/smoke.log 2>&1 || exit 1
timeout -k 10 600 python -u -m pytest tests -x -v -m gpu --timeout 120 --timeout-method thread > $O/pytest.log 2>&1 || exit 1
timeout -k 10 600 python -u bench.py --full --steps 5 --warmup 2 --no-cpu > $O/bench.log 2>&1 || exit 1
echo done
