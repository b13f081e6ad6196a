#!/bin/bash
# bench.py --full line + rocprofv3 kernel stats of the same bench (tag = $1); results under
# $OUT_DIR (default bench_out/)
set -o pipefail
tag=${1:-x}
O=${OUT_DIR:-bench_out}
mkdir -p $O
timeout -k 10 400 python bench.py --full --cpu-baseline 0 > $O/bench_$tag.json 2> $O/bench_$tag.err && \
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT && \
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_$tag -o run -- python bench.py --full --steps 8 --warmup 3 --cpu-baseline 0 > $O/prof_$tag.log 2>&1
echo "rc=$?" > $O/rc_$tag.txt
