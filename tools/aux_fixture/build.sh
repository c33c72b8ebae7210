#!/bin/bash
# Builds the auxiliary-GF / Jijk fixture driver against the compiled reference that build() leaves in oracle/_ref (librslmto_ref.a, mod/).
# Output: oracle/_ref/aux_driver.x (git-ignored with the rest of oracle/_ref: it holds reference object code).
set -euo pipefail
HERE="$(cd "$(dirname "$0")" && pwd)"
ROOT="$(dirname "$(dirname "$HERE")")"
REFOUT="$ROOT/oracle/_ref"
FC="${FC:-/opt/rocm/bin/amdflang}"
MKLDIR="${MKLDIR:-/opt/conda/lib}"
[ -f "$REFOUT/librslmto_ref.a" ] || { echo "oracle/_ref/librslmto_ref.a missing: run __graft_entry__.build() first" >&2; exit 1; }
mkdir -p "$REFOUT/aux_fixture"
cd "$REFOUT/aux_fixture"
"$FC" -cpp -O2 -fopenmp -I"$REFOUT/mod" -c "$HERE/aux_driver.f90" -o aux_driver.o
"$FC" aux_driver.o "$REFOUT/librslmto_ref.a" -fopenmp -L"$MKLDIR" -lmkl_rt -Wl,-rpath,"$MKLDIR" -o "$REFOUT/aux_driver.x"
echo "built $REFOUT/aux_driver.x"
