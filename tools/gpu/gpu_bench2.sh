#!/bin/bash
# Rehearsal of the driver's N = 2 bench on a one-GPU box: two ranks (torch.distributed.run) share the GPU and
# exchange tile sizes over the host (FRS_COMM_BACKEND=tcp; RCCL needs one GPU per rank).  -> $O/
set -o pipefail
cd "$GRAFT_REPO_ROOT"
export TMPDIR=/tmp FRS_COMM_BACKEND=tcp
O=${FRS_OUT:-$PWD/bench_out}/bench2
mkdir -p $O
timeout -k 10 400 python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 \
  --master-port 29711 bench.py --full --gpus 2 --steps 5 --warmup 2 ${BENCH_ARGS:-} > $O/bench.json 2> $O/bench.err || { tail -30 $O/bench.err; exit 1; }
cat $O/bench.json
