#!/bin/bash
# Packed against plain fp32 VALU issue cost (tools/ubench/pk_rate.hip): build if needed, run on the GPU, file the table.
#   usage: tools/ubench/pk_rate.sh [out.txt]        (default profiles/r09_pk_rate.txt)
set -e -o pipefail
cd "$(dirname "$0")/../.."
OUT=${1:-profiles/r09_pk_rate.txt}
[ -x tools/ubench/pk_rate ] && [ tools/ubench/pk_rate -nt tools/ubench/pk_rate.hip ] || hipcc --offload-arch=gfx950 -O3 -o tools/ubench/pk_rate tools/ubench/pk_rate.hip
mkdir -p "$(dirname "$OUT")"
timeout -k 10 120 tools/ubench/pk_rate | tee "$OUT"
