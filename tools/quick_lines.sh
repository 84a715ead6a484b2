#!/bin/bash
# One pfb line and one default (c5) line without CPU baselines: tools/quick_lines.sh TAG
set -e
TAG=${1:?tag}
OUT=${OUT:-out}            # where the pass leaves its files
cd "$(dirname "$0")/.." && mkdir -p $OUT
timeout -k 10 300 python3 bench.py --workload pfb --full --no-cpu-baseline > $OUT/${TAG}_pfb.json 2> $OUT/${TAG}_pfb.err
timeout -k 10 400 python3 bench.py --full --no-cpu-baseline > $OUT/${TAG}_bench.json 2> $OUT/${TAG}_bench.err
python3 - "$TAG" "$OUT" <<'PY'
import json, sys
t, out = sys.argv[1:3]
d = json.load(open(f"{out}/{t}_pfb.json"))
print("pfb", d["ms_per_step"], d["roofline"]["frac"], d["roofline"]["traffic_source"])
d = json.load(open(f"{out}/{t}_bench.json"))
print("c5", d["ms_per_step"], d["stages_ms"], d["stages_ghz"], d["stages_roofline_c2"]["fir+psd"]["hbm_frac"])
PY
