export RJ_OUT=${RJ_OUT:-bench_out}  # where the logs go
cd "$(dirname "$0")/.." && mkdir -p $RJ_OUT
for N in 2 4; do
  RJ_BENCH_SHARE_GPU=1 timeout -k 10 300 python3 -m torch.distributed.run --nnodes=1 --nproc-per-node $N --master-addr 127.0.0.1 --master-port $((29500 + N)) bench.py --full --gpus $N --steps 3 --warmup 1 --batch 128 > $RJ_OUT/share_n${N}.log 2>&1 || { echo "N=$N failed"; tail -20 $RJ_OUT/share_n${N}.log; exit 1; }
  grep '^{' $RJ_OUT/share_n${N}.log | tail -1 | cut -c1-600
done
