#!/bin/bash
cd "${GRAFT_REPO_ROOT:-.}"
o=${1:?usage: r06_bc.sh OUTPUT_DIR}; mkdir -p $o
for i in 1 2 3; do python3 bench.py --full --steps 30 --warmup 10 > $o/r06_bench.json 2> $o/r06_bench.err; python -c "import json; d=json.load(open(\"$o/r06_bench.json\")); print(d[\"ms_per_step\"], d[\"strong_scaling_ceiling\"][\"ms_per_step_of_each_engine\"], d[\"bs8_256\"][\"ms_per_step\"], d[\"h512_bs2\"][\"ms_per_step\"])"; done
tail -c 300 $o/r06_bench.json
python - $o/r06_bench.json <<'P'
import json, sys
d=json.load(open(sys.argv[1]))
print(d['ms_per_step'], d['strong_scaling_ceiling'])
P
