#!/bin/bash
# Round-end evidence refresh (run on the GPU box): PMC traffic passes, the
# bench lines of every model path (the training line reads the fresh PMC
# file), timed-region kernel profiles and the per-shape conv table.
# usage: tools/refresh_profiles.sh <round tag, e.g. r2>
set -eo pipefail
tag=$1
mkdir -p gpurun_out
bash tools/pmc_traffic.sh $tag --steps 3 --warmup 2
cp gpurun_out/${tag}_pmc.json profiles/${tag}_train_pmc.json
# (--full: these lines carry the box calibration, the fixed-rows region and the CPU baseline)
timeout -k 10 400 python3 bench.py --full | tail -1 > profiles/${tag}_train_bench_line.json
timeout -k 10 400 python3 bench.py --full --mode infer | tail -1 > profiles/${tag}_infer_bench_line.json
timeout -k 10 400 python3 bench.py --full --model retinanet_R_101_FPN --mode infer | tail -1 > profiles/${tag}_retinanet_bench_line.json
timeout -k 10 400 python3 bench.py --full --model solo_v2_R_50_FPN --mode infer | tail -1 > profiles/${tag}_solo_bench_line.json
bash tools/profile_bench.sh ${tag}_train --steps 5 --warmup 3
bash tools/profile_bench.sh ${tag}_solo --model solo_v2_R_50_FPN --mode infer --steps 5 --warmup 3
bash tools/profile_bench.sh ${tag}_retinanet --model retinanet_R_101_FPN --mode infer --steps 5 --warmup 3
timeout -k 10 300 python3 tools/conv_shapes.py > gpurun_out/${tag}_conv_shapes.txt 2>&1
for m in train infer retinanet solo; do cat profiles/${tag}_${m}_bench_line.json; done
