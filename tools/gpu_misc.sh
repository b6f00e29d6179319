#!/bin/bash
# GPU session: twins bench with its CPU baseline (--full), and a 2-rank bench
# rehearsal on one GPU (gloo) of the distributed exchange path.  Logs go to
# $BENCH_LOGS (default bench_logs/).
cd "$(dirname "$0")/.." || exit 2
LOGS=${BENCH_LOGS:-bench_logs}
mkdir -p "$LOGS"
export TMPDIR=/tmp
timeout -k 10 300 python -u bench.py --full --mode twins > "$LOGS/bench_twins_cpu.log" 2>&1 || exit $?
grep '^{' "$LOGS/bench_twins_cpu.log"
timeout -k 10 300 python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 \
  --master-port 29555 bench.py --gpus 2 --steps 5 --warmup 1 --dist-backend gloo --one-device \
  > "$LOGS/bench_2rank_gloo.log" 2>&1 || exit $?
grep '^{' "$LOGS/bench_2rank_gloo.log"
