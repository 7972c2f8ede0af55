#!/bin/bash
# GPU box: the -m gpu suite, then the bench line of the four interior workloads (stand-in and harder stand-in, 1080p and 4K).
#   tools/gpu_interiors.sh [TAG]      -> $OUT/TAG_pytest.txt, TAG_bench_<workload>.json  (OUT: default results)
tag=${1:-interiors}
OUT=${OUT:-results}; mkdir -p $OUT
python3 -m pytest tests -m gpu -x -q > $OUT/${tag}_pytest.txt 2>&1; tail -4 $OUT/${tag}_pytest.txt
for w in interior_hard_1080p_ao interior_hard_4k_ao interior_1080p_ao interior_4k_ao; do
  python3 bench.py --full --steps 20 --warmup 5 --workload $w --no-end-to-end > $OUT/${tag}_bench_$w.json 2> $OUT/${tag}_bench_$w.err
  python3 -c "
import json; d=json.load(open('$OUT/${tag}_bench_$w.json')); print('$w', d['value'], d['ms_per_step'], 'pipelined', d['pipelined']['value'], 'cpu', d['cpu_baseline']['value'], d['config']['rays_per_frame'])"
done
