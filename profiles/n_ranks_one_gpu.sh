#!/bin/bash
# bench.py --gpus N paths (row bands + gather leg, fanin with the auto / bands / spread plans) run by 2-3 processes on one GPU
# with --full (the gather leg and the parity checks): bash profiles/n_ranks_one_gpu.sh [output dir]   (from the repo root)
set -x
OUT=${1:-n_ranks_one_gpu_out}
mkdir -p $OUT
export MASTER_ADDR=127.0.0.1
timeout -k 10 300 python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29511 bench.py --full --gpus 2 --dist-backend gloo --steps 10 --warmup 3 --size 2048 > $OUT/r04_n2_rows.json 2> $OUT/r04_n2_rows.err; echo rc=$?
tail -3 $OUT/r04_n2_rows.err; cat $OUT/r04_n2_rows.json
for pol in auto bands spread; do
timeout -k 10 300 python -m torch.distributed.run --nnodes=1 --nproc-per-node 3 --master-addr 127.0.0.1 --master-port 29512 bench.py --full --gpus 3 --dist-backend gloo --workload fanin --policy $pol --steps 10 --warmup 3 --size 1024 > $OUT/r04_n3_fanin_$pol.json 2> $OUT/r04_n3_fanin_$pol.err; echo rc=$?
tail -3 $OUT/r04_n3_fanin_$pol.err; cat $OUT/r04_n3_fanin_$pol.json
done
