#!/bin/bash
# The first half of tools/round_pass.sh (one GPU call stays under gpurun's
# 20-minute limit): GPU suite, smoke, default bench (c5 + CPU baselines + the
# c2 FIR+PSD leg), c2 / sync / pfb lines, rocprofv3 kernel stats of the
# default workload.  Usage: tools/round_pass_a.sh TAG
set -e
TAG=${1:?tag}
OUT=${OUT:-out}            # where the pass leaves its files
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
mkdir -p $OUT
timeout -k 10 600 python -u -m pytest tests -m gpu -x -v --timeout 120 --timeout-method thread > $OUT/${TAG}_gputests.txt 2>&1 || { tail -30 $OUT/${TAG}_gputests.txt; exit 1; }
tail -2 $OUT/${TAG}_gputests.txt
timeout -k 10 200 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/${TAG}_smoke.txt 2>&1
tail -1 $OUT/${TAG}_smoke.txt
timeout -k 10 400 python3 bench.py --full > $OUT/${TAG}_bench.json 2> $OUT/${TAG}_bench.err
cat $OUT/${TAG}_bench.json
for w in c2 sync pfb; do
  timeout -k 10 300 python3 bench.py --workload $w --full --no-cpu-baseline > $OUT/${TAG}_$w.json 2> $OUT/${TAG}_$w.err
  cat $OUT/${TAG}_$w.json
done
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/${TAG}_prof -o run -- python3 bench.py --steps 10 --no-cpu-baseline --no-c2-leg > $OUT/${TAG}_prof.log 2>&1
python3 tools/db_stats.py $OUT/${TAG}_prof/run_results.db $OUT/${TAG}_kernel_stats.csv > /dev/null
rm -rf $OUT/${TAG}_prof          # the raw traces are large; the table above is what is kept
echo prof done
