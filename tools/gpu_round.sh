# One gpurun call: GPU tests, the default bench line, rocprofv3 kernel stats of both
# workloads.  Everything lands under gpurun_out/$TAG/.
#   gpurun --timeout 1500 -- 'bash tools/gpu_round.sh r02a [tests|bench|prof|pmc ...]'
TAG=${1:-cur}; shift
WHAT=${@:-tests bench prof}
R=$GRAFT_REPO_ROOT
OUT=$R/gpurun_out/$TAG
mkdir -p $OUT
cd $R
for w in $WHAT; do
  case $w in
    tests)
      timeout 1200 python -m pytest tests -m gpu -x -q 2>&1 | tail -40 > $OUT/gpu_tests.log
      tail -3 $OUT/gpu_tests.log ;;
    tests_all)   # no -x: every failure listed
      timeout 1500 python -m pytest tests -m gpu -q 2>&1 | tail -150 > $OUT/gpu_tests.log
      tail -3 $OUT/gpu_tests.log ;;
    bench)
      timeout 600 python bench.py --full > $OUT/bench_default.json 2> $OUT/bench_default.err
      tail -c 600 $OUT/bench_default.json; tail -3 $OUT/bench_default.err ;;
    prof)
      for wl in lc transfusion_l; do bash $R/tools/prof_bench.sh $TAG $wl; done ;;
    rb)   # integer kernels at nominal and stress size (profiles/rNN_rulebook_voxelize_roofline.jsonl)
      timeout 300 python tools/rulebook_bench.py 2>/dev/null > $OUT/rulebook_voxelize_roofline.jsonl
      cut -c1-200 $OUT/rulebook_voxelize_roofline.jsonl
      timeout 120 python tools/fps_bench.py 2>/dev/null | grep -v amdgpu.ids > $OUT/fps.txt; cat $OUT/fps.txt ;;
    cpu2)   # one rank on the two CPUs plan_rank_cpus grants at 8 ranks per 16-CPU node
      MSMD_PIN_CPUS=0,1 MSMD_CPU_QUOTA=2 timeout 300 taskset -c 0,1 python bench.py --full --no-also --no-cpu-baseline > $OUT/bench_2cpu.json 2> $OUT/bench_2cpu.err
      timeout 300 python bench.py --full --no-also --no-cpu-baseline > $OUT/bench_4cpu.json 2> $OUT/bench_4cpu.err
      python -c "
import json
for n in ('2cpu', '4cpu'):
    d = json.load(open('$OUT/bench_%s.json' % n)); print(n, d['value'], d['ms_per_step'], d['host'])" ;;
    pmc)
      bash tools/pmc_collect.sh lc $OUT/pmc_lc
      bash tools/pmc_collect.sh transfusion_l $OUT/pmc_transfusion_l ;;
  esac
done
