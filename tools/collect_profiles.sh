#!/bin/bash
# the per-round evidence in one call (run on the GPU box): kernel stats of `bench.py --full --no-extras` under
# rocprofv3, the four PMC traffic passes (-> profiles/pmc_traffic.json with the sources' hashes and SPMV_COMMIT), the full bench line.
# Outputs go to $SPMV_PROFILE_OUT (default: profile_out/ in the repository).
# usage: SPMV_COMMIT=<hash> tools/collect_profiles.sh r04
TAG=${1:-r04}
R="$(cd "$(dirname "$0")/.." && pwd)"
OUT=${SPMV_PROFILE_OUT:-$R/profile_out}
cd /tmp && export TMPDIR=/tmp
mkdir -p $OUT/${TAG}_stats
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/${TAG}_stats -o $TAG -- python3 $R/bench.py --full --no-extras > $OUT/${TAG}_bench_under_rocprof.json 2> $OUT/${TAG}_bench_under_rocprof.err || exit 1
echo "stats done"
SPMV_PROFILE_OUT=$OUT bash $R/tools/pmc_traffic.sh || exit 1
cd $R && SPMV_PROFILE_OUT=$OUT python3 tools/pmc_traffic.py && cp profiles/pmc_traffic.json $OUT/pmc_traffic_${TAG}.json
timeout -k 10 600 python3 bench.py --full > $OUT/${TAG}_bench_line.json 2> $OUT/${TAG}_bench_line.err; echo "bench rc=$?"
