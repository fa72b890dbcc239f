#!/bin/bash
# MIP against the composite kernel (tools/mip_bench.py) for C2, C3 and C4 on the GPU box: one
# process per configuration, each under its own time limit, chained with && (the first failure
# ends the script).  Usage: bash tools/mip_bench.sh [output directory, default profiles/r07/mip]
set -o pipefail
O=${1:-profiles/r07/mip}
mkdir -p $O
timeout -k 10 150 python tools/mip_bench.py --config c2 --out $O &&
timeout -k 10 240 python tools/mip_bench.py --config c3 --out $O &&
timeout -k 10 420 python tools/mip_bench.py --config c4 --out $O
