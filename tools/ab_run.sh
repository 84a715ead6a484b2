#!/bin/bash
# A/B of library builds on one bench line: tools/ab_run.sh TAG "bench args" lib1 lib2 ...
# (each lib: vector_amd/<name>.so built by _build.build(defines=..., out=...); "base" = libvsig.so)
set -e
TAG=$1; ARGS=$2; shift 2
OUT=${OUT:-out}            # where the runs leave their lines
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
mkdir -p $OUT
for lib in "$@"; do
  if [ "$lib" = base ]; then unset VSIG_LIB; else export VSIG_LIB=$GRAFT_REPO_ROOT/vector_amd/$lib.so; fi
  timeout -k 10 240 python3 bench.py $ARGS --full --no-cpu-baseline > $OUT/${TAG}_$lib.json 2> $OUT/${TAG}_$lib.err
  python3 -c "import json,sys; d=json.load(open('$OUT/${TAG}_$lib.json')); print('$lib', d['ms_per_step'], d.get('stages_ms'), d.get('stages_ghz'), d['check']['ok'])"
done
