# Parity suite + bench + SQ counters of the product library at HEAD (one GPU call).
#   bash scripts/gpu_quick_ab.sh TAG   -> $OUT/{pytest_TAG.txt, bench_TAG.json, sq_TAG.txt}   (OUT: default bench_out)
set -o pipefail
cd /root/repo
export TMPDIR=/tmp
T=${1:-head}
OUT=${OUT:-bench_out}
mkdir -p $OUT
timeout -k 10 600 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread > $OUT/pytest_$T.txt 2>&1 && \
for r in 1 2 3; do timeout -k 10 120 python bench.py --full --no-cpu-baseline --no-controller --steps 100 --warmup 20 || exit 1; done > $OUT/bench_$T.json 2>/dev/null && \
for r in 1 2; do timeout -k 10 120 python bench.py --full --horizon 20 --no-cpu-baseline --no-controller --steps 50 --warmup 5 || exit 1; done >> $OUT/bench_$T.json 2>/dev/null && \
bash scripts/gpu_sq_ab.sh $T= > $OUT/sq_$T.log 2>&1
