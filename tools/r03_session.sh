#!/bin/bash
# Round-3 GPU session: each GPU step under its own time limit; a crash / timeout ends the session
# (a plain test failure, exit 1, does not).  STEPS picks the steps; logs under gpurun_out/.
set -u
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
mkdir -p gpurun_out
export TMPDIR=/tmp PYTHONDONTWRITEBYTECODE=1
TAG=${TAG:-r03}
run() { local name=$1 to=$2; shift 2; echo "== $name $(date +%T)"; timeout -k 10 "$to" "$@" > "gpurun_out/$name.log" 2>&1; local rc=$?
        echo "$name rc=$rc"; tail -4 "gpurun_out/$name.log"; if [ $rc -ne 0 ] && [ $rc -ne 1 ]; then exit $rc; fi; }
for step in ${STEPS:-pytest smoke bench}; do
  case $step in
    pytest) run pytest_gpu 1100 python3 -u -m pytest tests -m gpu -x -v --timeout 120 --timeout-method thread ;;
    pyfiles) run pytest_files 1100 python3 -u -m pytest ${FILES} -x -v --timeout 120 --timeout-method thread ;;
    smoke) run smoke 300 python3 -c "import __graft_entry__ as g; g.smoke()" ;;
    bench) run bench 300 python3 bench.py --full ;;
    secondary)
      : > gpurun_out/secondary.jsonl
      for wl in ${WL:-sign sign256 qsgd terngrad powersgd}; do
        st=20; case $wl in sign|powersgd|ddp_segmented|qsgd|terngrad|qsgd_step|terngrad_step) st=200;; esac
        run "bench_$wl" 300 python3 bench.py --workload $wl --steps $st --no-cpu-baseline
        grep '^{' "gpurun_out/bench_$wl.log" | tail -1 >> gpurun_out/secondary.jsonl
      done ;;
    prof) run prof_topk 300 rocprofv3 --kernel-trace --stats --output-format csv -d gpurun_out/prof_${TAG}_topk -o run \
            -- python3 bench.py --steps 10 --warmup 3 --no-cpu-baseline ;;
    profwl) for wl in ${PROF_WL:-powersgd terngrad qsgd sign}; do
              st=20; run "prof_$wl" 300 rocprofv3 --kernel-trace --stats --output-format csv -d gpurun_out/prof_${TAG}_$wl -o run \
                -- python3 bench.py --workload $wl --steps $st --warmup 5 --no-cpu-baseline
            done ;;
    exp) run exp 600 python3 ${EXP} ;;
  esac
done
