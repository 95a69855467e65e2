# Round-3 profile collection (run through gpurun from the repo root): rocprofv3 kernel stats of the bench step and of the batch-1 chunk, then the
# two PMC passes of the dominant GEMM shape.  Counters are collected in their own runs (--pmc with --kernel-trace only).
OUT=$(realpath -m "${1:?usage: tools/r03_profiles.sh OUTDIR}")
cd /tmp && export TMPDIR=/tmp
R=$GRAFT_REPO_ROOT
mkdir -p $OUT
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/bench -o b -- python3 $R/bench.py --steps 10 --warmup 3 --full --no-eager-baseline --no-cpu-baseline --no-inference > $OUT/bench_under_rocprof.json 2> $OUT/bench.err
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/infer -o ip -- python3 $R/tools/infer_profile.py > $OUT/infer.log 2>&1
bash $R/tools/pmc_traffic.sh > $OUT/pmc.log 2>&1
echo profiles-done
