# round 5: GPU test-suite + default bench line of the product build
cd $GRAFT_REPO_ROOT
OUT=${1:?usage: bash tools/gpu/r05b.sh OUTDIR}
mkdir -p "$OUT" && OUT=$(cd "$OUT" && pwd)
timeout 3000 python -m pytest tests -m gpu -x -q 2>&1 | tail -15 > $OUT/pytest_gpu.txt
cat $OUT/pytest_gpu.txt
timeout 900 python bench.py --full --steps 20 --warmup 5 > $OUT/bench_default.json 2> $OUT/bench_default.err
tail -1 $OUT/bench_default.json | cut -c1-1500
