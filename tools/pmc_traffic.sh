#!/bin/bash
# tools/pmc_traffic.sh -- HBM traffic of the hot kernels from rocprofv3 PMC counters (run on the GPU box):
#   separate --pmc passes for FETCH_SIZE and WRITE_SIZE (they do not fit one pass), kernel-trace only.
# Writes $TMPDIR/pmc_traffic_{FETCH_SIZE,WRITE_SIZE}/ ; tools/pmc_traffic.py turns them into profiles/pmc_traffic.json.
# --full: the store-path region (index_max_gather, som_group) runs only there; the --no-* flags keep the run to a few steps.
R=${GRAFT_REPO_ROOT:-$(pwd)}
export TMPDIR=${TMPDIR:-/tmp} && cd $TMPDIR     # (tools/pmc_traffic.py reads the passes from the same place)
for c in FETCH_SIZE WRITE_SIZE; do
  rocprofv3 --pmc $c --kernel-trace --output-format csv -d $TMPDIR/pmc_traffic_$c -o pmc -- python $R/bench.py --steps 3 --warmup 1 --full --no-cpu-baseline --no-graph --no-other-precisions --no-parity-check --no-other-configs $EXTRA > /dev/null 2> $TMPDIR/pmc_traffic_$c.err
done
