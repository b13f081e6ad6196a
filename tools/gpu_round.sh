set -o pipefail
O=${OUT_DIR:-bench_out}
mkdir -p $O
timeout -k 10 900 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread > $O/gpu_tests.log 2>&1 && \
timeout -k 10 400 python bench.py --full > $O/bench.json 2> $O/bench.err && \
timeout -k 10 120 python tools/coatt_bench.py > $O/coatt.log 2>&1 && \
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT && \
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof8 -o run -- python bench.py --full --steps 8 --warmup 3 --cpu-baseline 0 > $O/prof8.log 2>&1
