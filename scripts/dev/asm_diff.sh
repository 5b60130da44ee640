#!/bin/bash
# Device code of two checkouts, file by file: scripts/dev/asm_diff.sh <checkout A> <checkout B> [-DLQ_STAMPS ...] [-- file.hip ...]
# Compiles every csrc/*.hip of both (or only the files named after `--`) with the Makefile's FLAGS to device assembly and compares it
# without the per-compilation __hip_cuid_ lines.  "same" for every file = not one instruction differs.  No GPU needed (about 40 s
# per file, side and core; lipvq_fused.hip: 3 min).  "FAILED <file>": hipcc failed on either side, or a file with __global__ functions
# gave no .amdhsa_kernel -- nothing was compared.  Exit status 0 only if every file is "same".
set -u
A=$1; B=$2; shift 2
DEFS=(); FILES=()
while [ $# -gt 0 ]; do
    if [ "$1" = "--" ]; then shift; FILES=("$@"); break; fi
    DEFS+=("$1"); shift
done
if [ ${#FILES[@]} -eq 0 ]; then for f in "$A"/lipvq-vae_amd/csrc/*.hip; do FILES+=("$(basename "$f")"); done; fi
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -fhip-fp32-correctly-rounded-divide-sqrt -fno-slp-vectorize"
TMP=$(mktemp -d); trap 'rm -rf "$TMP"' EXIT
# asm <checkout> <file> <out>: 0 if hipcc succeeded and the output has the kernels its source promises
asm() {
    (cd "$1/lipvq-vae_amd/csrc" && ${HIPCC:-/opt/rocm/bin/hipcc} $FLAGS ${DEFS[@]+"${DEFS[@]}"} --cuda-device-only -S -o - "$2" 2>"$3.err") | grep -v __hip_cuid_ >"$3"
    [ "${PIPESTATUS[0]}" -eq 0 ] || { cat "$3.err" >&2; return 1; }
    ! grep -q __global__ "$1/lipvq-vae_amd/csrc/$2" || grep -q '\.amdhsa_kernel' "$3"
}
rc=0
for f in "${FILES[@]}"; do
    asm "$A" "$f" "$TMP/a.s"; sa=$?
    asm "$B" "$f" "$TMP/b.s"; sb=$?
    if [ $sa -ne 0 ] || [ $sb -ne 0 ]; then echo "FAILED  $f ${DEFS[*]-}"; rc=1
    elif cmp -s "$TMP/a.s" "$TMP/b.s"; then echo "same    $f ${DEFS[*]-}"
    else echo "DIFFERS $f ${DEFS[*]-}"; rc=1; fi
done
exit $rc
