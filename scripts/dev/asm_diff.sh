#!/bin/bash
# Device code of two checkouts, file by file: scripts/dev/asm_diff.sh <checkout A> <checkout B> [-DLQ_STAMPS ...]
# Compiles every csrc/*.hip of both with the Makefile's FLAGS to device assembly and compares it without the per-compilation
# __hip_cuid_ lines.  "same" for every file = not one instruction differs.  No GPU needed (about 40 s per file and core).
set -u
A=$1; B=$2; shift 2
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -fhip-fp32-correctly-rounded-divide-sqrt -fno-slp-vectorize"
asm() { (cd "$1/lipvq-vae_amd/csrc" && ${HIPCC:-/opt/rocm/bin/hipcc} $FLAGS "${@:3}" --cuda-device-only -S -o - "$2" 2>/dev/null | grep -v __hip_cuid_); }
for f in "$A"/lipvq-vae_amd/csrc/*.hip; do
    f=$(basename "$f")
    if cmp -s <(asm "$A" "$f" "$@") <(asm "$B" "$f" "$@"); then echo "same    $f $*"; else echo "DIFFERS $f $*"; fi
done
