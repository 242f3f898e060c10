# GPU-box driver: kernel numerics, parity, smoke, bench, rocprof.  Usage: bash tests/run_gpu_suite.sh [stage...]
REPO=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p "${OUT:=$REPO/out}"; OUT=$(cd "$OUT" && pwd)     # OUT: where logs, JSON lines and profiles go
STAGES="${@:-kernels parity smoke bench prof}"
ok=1
for st in $STAGES; do
  [ $ok -eq 1 ] || break
  case $st in
    kernels) timeout -k 10 600 python -m pytest tests/test_gpu_kernels.py -m gpu -q -p no:cacheprovider -x > $OUT/pytest_kernels.log 2>&1; rc=$?; tail -15 $OUT/pytest_kernels.log;;
    fold)    timeout -k 10 900 python -m pytest tests/test_gpu_fold.py tests/test_gpu_batch_sweep.py -m gpu -q -p no:cacheprovider > $OUT/pytest_fold.log 2>&1; rc=$?; tail -40 $OUT/pytest_fold.log;;
    gemm)    timeout -k 10 300 python -m pytest tests/test_gpu_gemm_edges.py -m gpu -q -p no:cacheprovider > $OUT/pytest_gemm.log 2>&1; rc=$?; tail -40 $OUT/pytest_gemm.log;;
    mx)      timeout -k 10 300 python -m pytest tests/test_gpu_mx_exact.py -m gpu -q -p no:cacheprovider > $OUT/pytest_mx.log 2>&1; rc=$?; tail -40 $OUT/pytest_mx.log;;
    all)     timeout -k 10 1150 python -m pytest tests -m gpu -q -p no:cacheprovider > $OUT/pytest_all.log 2>&1; rc=$?; tail -40 $OUT/pytest_all.log;;
    benchq)  timeout -k 10 600 python bench.py --full --steps 3 --warmup 1 --cpu-steps 0 --no-nar --no-nq8 --no-fp8 --no-vctk 2> $OUT/benchq.err | tee $OUT/benchq.json; rc=${PIPESTATUS[0]}; tail -5 $OUT/benchq.err;;
    profab)  cd /tmp && export TMPDIR=/tmp; rc=0
             for arm in ${PROF_ARMS:-ln_fold=1 ln_fold=0}; do
               tag=$(echo "$arm" | tr ',=' '__')
               timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_$tag -- python3 $REPO/bench.py --steps 1 --warmup 1 --cpu-steps 0 --no-latency --no-nar --no-nq8 --no-fp8 --no-vctk --no-kernel-events --profile-iters 24 --tune "$arm" ${PROF_EXTRA:-} > $OUT/prof_$tag.log 2>&1 || rc=$?
               f=$(find $OUT/prof_$tag -name "*kernel_stats.csv" | head -1)
               echo "== $arm"; python3 $REPO/tools/show_kernel_stats.py "$f" 22
               cp "$f" $OUT/kernel_stats_$tag.csv
             done; cd $REPO;;
    parity)  timeout -k 10 900 python -m pytest tests/test_gpu_parity.py -m gpu -q -p no:cacheprovider > $OUT/pytest_parity.log 2>&1; rc=$?; tail -25 $OUT/pytest_parity.log;;
    nar)     timeout -k 10 600 python -m pytest tests/test_gpu_nar.py -m gpu -q -p no:cacheprovider > $OUT/pytest_nar.log 2>&1; rc=$?; tail -25 $OUT/pytest_nar.log;;
    smoke)   timeout -k 10 180 python __graft_entry__.py --smoke > $OUT/smoke.log 2>&1; rc=$?; tail -3 $OUT/smoke.log;;
    bench)   timeout -k 10 900 python bench.py --full --steps 2 --warmup 1 2> $OUT/bench.err | tee $OUT/bench.json; rc=${PIPESTATUS[0]}; tail -5 $OUT/bench.err;;
    noev)    timeout -k 10 600 python bench.py --steps 2 --warmup 1 --no-kernel-events --cpu-steps 0 --no-vctk --no-nq8 --no-latency --no-fp8 2> $OUT/bench_noev.err | tee $OUT/bench_noev.json; rc=${PIPESTATUS[0]};;
    streams) rc=0; for k in 1 2 4; do timeout -k 10 300 python bench.py --full --steps 2 --warmup 1 --cpu-steps 0 --no-vctk --no-nq8 --no-latency --no-fp8 --streams $k 2>> $OUT/bench_streams.err | tee -a $OUT/bench_streams.json || rc=$?; done;;
    dp2)     timeout -k 10 300 python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29511 bench.py --full --gpus 2 --steps 1 --warmup 1 --backend gloo --batch 4 --profile-iters 3 --cpu-steps 0 --no-vctk --no-nq8 --no-latency --no-nar --no-fp8 2> $OUT/bench_dp2.err | tee $OUT/bench_dp2.json; rc=${PIPESTATUS[0]}; tail -3 $OUT/bench_dp2.err;;
    micro)   timeout -k 10 600 python tests/bench_kernels.py > $OUT/kernels.txt 2> $OUT/kernels.err; rc=$?; cat $OUT/kernels.txt;;
    pmc)     cd /tmp && export TMPDIR=/tmp; rc=0
             for c in FETCH_SIZE WRITE_SIZE; do
               timeout -k 10 500 rocprofv3 --pmc $c --kernel-trace --output-format csv -d $OUT/pmc_$c -- python3 $REPO/bench.py --full --steps 1 --warmup 0 --cpu-steps 0 --no-vctk --no-nq8 --no-latency --no-nar --no-fp8 --profile-iters 3 > $OUT/pmc_$c.log 2>&1 || rc=$?
               echo "pmc $c rc=$rc"
             done; cd $REPO; find $OUT/pmc_* -name "*.csv" | head;;
    prof1)   cd /tmp && export TMPDIR=/tmp && timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof1 -- python3 $REPO/bench.py --full --batch 1 --steps 5 --warmup 1 --cpu-steps 0 --no-vctk --no-nq8 --no-latency > $OUT/prof1.log 2>&1; rc=$?; cd $REPO; tail -2 $OUT/prof1.log;;
    prof)    cd /tmp && export TMPDIR=/tmp && timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof -- python3 $REPO/bench.py --full --steps 1 --warmup 1 --cpu-steps 0 --no-vctk --no-nq8 --no-latency --no-nar > $OUT/prof.log 2>&1; rc=$?; cd $REPO; tail -3 $OUT/prof.log; find $OUT/prof -name "*stats*" | head;;
  esac
  echo "stage $st rc=$rc"
  if [ $rc -eq 124 ] || [ $rc -eq 137 ]; then ok=0; fi
done
