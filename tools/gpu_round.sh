# GPU evidence for the current tree: GPU tests, the full bench line, rocprofv3 kernel stats of the bench.
# usage: [OUT=dir] bash tools/gpu_round.sh TAG     (logs go to $OUT, default ./out)
set -o pipefail
R=${GRAFT_REPO_ROOT:-$(pwd)}
TAG=${1:-r01}
OUT=$(realpath -m "${OUT:-$R/out}")     # absolute: the profiler pass below runs elsewhere
mkdir -p $OUT
cd $R
timeout -k 10 600 python -u -m pytest tests -m gpu -x -v --timeout 300 --timeout-method thread > $OUT/${TAG}_gpu_tests.log 2>&1; rc=$?
tail -n 5 $OUT/${TAG}_gpu_tests.log
[ $rc -ne 0 ] && exit $rc
timeout -k 10 600 python bench.py --full > $OUT/${TAG}_bench.log 2>&1 || exit $?
grep -v amdgpu.ids $OUT/${TAG}_bench.log | cut -c1-3000
export TMPDIR=/tmp
cd /tmp
timeout -k 10 500 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/${TAG}_kt -o run -- python3 $R/bench.py --full --steps 2 --warmup 1 --no-cpu-baseline > $OUT/${TAG}_kt.log 2>&1 || exit $?
