# The whole GPU suite, then the full bench line and a configs4-rank line.
# usage: [OUT=dir] bash tools/gpu_full.sh TAG     (logs go to $OUT, default ./out)
set -o pipefail
R=${GRAFT_REPO_ROOT:-$(pwd)}
TAG=${1:-full}
OUT=$(realpath -m "${OUT:-$R/out}")     # absolute: the runs below start from $R
mkdir -p $OUT
cd $R
timeout -k 10 900 python -u -m pytest tests -m gpu -x -v --timeout 300 --timeout-method thread > $OUT/${TAG}_gpu_tests.log 2>&1 || { tail -40 $OUT/${TAG}_gpu_tests.log; exit 1; }
tail -n 3 $OUT/${TAG}_gpu_tests.log
timeout -k 10 600 python bench.py --full > $OUT/${TAG}_bench.log 2>&1 || { tail -30 $OUT/${TAG}_bench.log; exit 1; }
grep -v amdgpu.ids $OUT/${TAG}_bench.log | cut -c1-1200
timeout -k 10 400 python bench.py --full --workload configs4-rank --steps 1 --warmup 1 > $OUT/${TAG}_c4.log 2>&1 || { tail -30 $OUT/${TAG}_c4.log; exit 1; }
grep -v amdgpu.ids $OUT/${TAG}_c4.log | cut -c1-1500
if [ "$2" = "mhap" ]; then
  timeout -k 10 600 python bench_mhap.py > $OUT/${TAG}_mhap.log 2>&1 || { tail -30 $OUT/${TAG}_mhap.log; exit 1; }
  grep -v amdgpu.ids $OUT/${TAG}_mhap.log | cut -c1-2500
fi
