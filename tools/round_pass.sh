#!/bin/bash
# One GPU pass: GPU suite, smoke, default bench (c5 + CPU baseline + the c2
# FIR+PSD leg), c2 / sync / pfb bench lines, rocprofv3 kernel stats of the
# default workload; with PMC=1 also the counter passes of c5, c2 and sync
# (tools/pmc.sh; summarise locally with tools/pmc_summary.py).
# Usage: [PMC=1] tools/round_pass.sh TAG
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
if [ "${PMC:-0}" = 1 ]; then
  mkdir -p $OUT/${TAG}_pmcsum
  pmc() {   # name keyspec bench-args...
    local name=$1 key=$2; shift 2
    bash tools/pmc.sh $OUT/${TAG}_pmc_$name "$@"
    python3 tools/pmc_summary.py $OUT/${TAG}_pmc_$name $OUT/${TAG}_pmcsum/pmc_${name}_${TAG}.json "$key" > /dev/null
    rm -rf $OUT/${TAG}_pmc_$name
  }
  pmc c5 n=2147483648:ntaps=255:decim=4:nfft=8192:L=4096 --no-c2-leg
  pmc c2 n=268435456:ntaps=255:decim=1:nfft=8192:L=4096 --workload c2
  pmc sync n=1073741824:L=4096 --workload sync
  echo pmc done
fi
echo done
