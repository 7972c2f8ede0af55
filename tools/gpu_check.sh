#!/bin/bash
# One GPU session's worth of checking (repo root): the -m gpu suite, an A/B of library builds on four workloads, the bench line.
#   tools/gpu_check.sh TAG [lib_a lib_b ...]      -> $OUT/TAG_pytest.txt, TAG_ab.txt, TAG_bench.json  (OUT: default results)
tag=${1:-check}; shift
variants=${@:-lib}
OUT=${OUT:-results}; mkdir -p $OUT
python3 -m pytest tests -m gpu -x -q > $OUT/${tag}_pytest.txt 2>&1; tail -5 $OUT/${tag}_pytest.txt
python3 tools/ab_variants.py $variants -- bunny_1080p_ao bunny_1080p_primary interior_1080p_ao bunny_600_defaults --reps 2 > $OUT/${tag}_ab.txt 2>&1; cat $OUT/${tag}_ab.txt
python3 bench.py --full --steps 20 --warmup 5 > $OUT/${tag}_bench.json 2> $OUT/${tag}_bench.err; tail -c 1500 $OUT/${tag}_bench.err
python3 -c "
import json; d=json.load(open('$OUT/${tag}_bench.json')); print('value', d['value'], 'ms', d['ms_per_step'], 'pipelined', d['pipelined']['value'], d.get('end_to_end'))"
