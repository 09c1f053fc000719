# the round's GPU evidence in ONE gpurun call on the final sources: full GPU test-suite, rocprofv3 summaries (row log + dense), C5 kernel
# trace, fwg_gae trace, bench lines
cd $GRAFT_REPO_ROOT
OUT=${1:?usage: bash tools/gpu/r06_final.sh OUTDIR}
mkdir -p "$OUT" && OUT=$(cd "$OUT" && pwd)
( time timeout 3000 python -m pytest tests -m gpu -q -p no:cacheprovider ) 2>&1 | tail -12 > $OUT/pytest_gpu.txt
cat $OUT/pytest_gpu.txt
bash tests/run_profile.sh r06 > $OUT/profile.log 2>&1
bash tests/run_profile.sh r06_dense --obs-layout dense > $OUT/profile_dense.log 2>&1
bash tests/run_profile_fused.sh > $OUT/profile_fused.log 2>&1
( R=$PWD && cd /tmp && export TMPDIR=/tmp && timeout 170 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/gae_trace -o trace -- python3 $R/tests/prof_gae.py > $OUT/gae.txt 2>&1 )
grep -h "k_gae" $OUT/gae_trace/*/*kernel_stats.csv $OUT/gae_trace/*kernel_stats.csv 2>/dev/null | head -3 >> $OUT/gae.txt
rm -rf $OUT/gae_trace
timeout 900 python bench.py --full --steps 20 --warmup 5 > $OUT/bench_default.json 2> $OUT/bench_default.err
timeout 900 python bench.py --full > $OUT/bench_noflags.json 2> $OUT/bench_noflags.err
timeout 300 python bench.py --workload c5 --steps 20 --warmup 4 --no-cpu-baseline > $OUT/bench_c5.json 2> $OUT/bench_c5.err
timeout 300 python bench.py --steps 2000 --warmup 200 --no-cpu-baseline --no-side > $OUT/bench_2000.json 2> $OUT/bench_2000.err
ls -la gpurun_out/prof_r06 gpurun_out/prof_r06_dense gpurun_out/prof_fused 2>/dev/null | head -30
tail -3 $OUT/gae.txt
tail -1 $OUT/bench_default.json | cut -c1-600
