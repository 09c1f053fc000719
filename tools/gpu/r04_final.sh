# the round's final GPU evidence: full GPU test-suite, rocprofv3 summaries (row log + dense), C5 kernel trace, bench lines
cd $GRAFT_REPO_ROOT
OUT=${1:?usage: bash tools/gpu/r04_final.sh OUTDIR}
mkdir -p "$OUT" && OUT=$(cd "$OUT" && pwd)
timeout 2400 python -m pytest tests -m gpu -x -q 2>&1 | tail -6 > $OUT/pytest_gpu.txt
cat $OUT/pytest_gpu.txt
bash tests/run_profile.sh r04 > $OUT/profile.log 2>&1
bash tests/run_profile.sh r04_dense --obs-layout dense > $OUT/profile_dense.log 2>&1
bash tests/run_profile_fused.sh > $OUT/profile_fused.log 2>&1
timeout 900 python bench.py --full --steps 20 --warmup 5 > $OUT/bench_default.json 2> $OUT/bench_default.err
timeout 300 python bench.py --workload c5 --steps 20 --warmup 4 --no-cpu-baseline > $OUT/bench_c5.json 2> $OUT/bench_c5.err
timeout 300 python bench.py --steps 2000 --warmup 200 --no-cpu-baseline --no-side > $OUT/bench_2000.json 2> $OUT/bench_2000.err
(cat /sys/fs/cgroup/cpu.max /sys/fs/cgroup/cpu/cpu.cfs_quota_us /sys/fs/cgroup/cpu/cpu.cfs_period_us; nproc; grep -c processor /proc/cpuinfo) > $OUT/host_cpus.txt 2>&1
TL_LIB=libfwgym_tl_log.so TL_WL=c3:log TL_STAGGER=2000 TL_PERM=1 timeout 300 python tools/timeline.py run 2>&1 | grep -v Warn > $OUT/timeline_log.txt
TL_LIB=libfwgym_tl_dense.so TL_WL=c3:dense TL_STAGGER=2000 TL_PERM=1 timeout 300 python tools/timeline.py run 2>&1 | grep -v Warn > $OUT/timeline_dense.txt
TL_LIB=libfwgym_tl_c5.so timeout 300 python tools/timeline_rollout.py 2>&1 | grep -v Warn > $OUT/timeline_rollout.txt
ls -la gpurun_out/prof_r04 gpurun_out/prof_r04_dense gpurun_out/prof_fused 2>/dev/null | head -30
tail -3 $OUT/bench_default.json | cut -c1-600
