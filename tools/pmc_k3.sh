#!/bin/bash
# development: HBM traffic of the contraction kernel (K3 / K3h) under the bench command -- FETCH_SIZE and WRITE_SIZE in separate
# --pmc passes, counters alone (no tracing), collected for the contraction kernels only; the text summary holds the means per
# dispatch that profiles/k3_traffic.json is filled in from (bytes_per_launch = 2 x FETCH_SIZE + WRITE_SIZE, in KB x 1024).
# usage (GPU box, repo root): tools/pmc_k3.sh <tag> [bench args...]      DDP_HIP_LIB selects an A/B build
set -e
ROOT=$(pwd); TAG=${1:-k3}; shift || true
OUT=${OUT:-build/pmc}     # where the logs and the summary go (relative to the repo root)
mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
for C in FETCH_SIZE WRITE_SIZE; do
  rm -rf /tmp/pmc_k3_${TAG}_$C
  timeout -k 10 400 rocprofv3 --pmc $C --kernel-include-regex bwd_contract --output-format csv -d /tmp/pmc_k3_${TAG}_$C -- python3 $ROOT/bench.py --gpus 1 --steps 1 --warmup 1 --no-extra --no-cpu-baseline --no-kernel-events "$@" > $ROOT/$OUT/k3_${TAG}_$C.log 2>&1
done
cd $ROOT
python3 tools/summarize_profile.py $OUT/summary_pmc_k3_$TAG.txt --pmc /tmp/pmc_k3_${TAG}_FETCH_SIZE --pmc /tmp/pmc_k3_${TAG}_WRITE_SIZE --filter "bwd_contract" \
  --note "rocprofv3 --pmc <counter> --kernel-include-regex bwd_contract -- python3 bench.py --gpus 1 --steps 1 --warmup 1 --no-extra --no-cpu-baseline --no-kernel-events $*: FETCH_SIZE and WRITE_SIZE in passes of their own, mean per dispatch" > /dev/null
grep "bwd_contract" $OUT/summary_pmc_k3_$TAG.txt | cut -c1-220
