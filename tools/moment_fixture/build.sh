#!/bin/bash
# Builds the moment-integral fixture driver against the compiled reference that build() leaves in oracle/_ref (librslmto_ref.a, mod/).
# Output: oracle/_ref/moment_driver.x (git-ignored with the rest of oracle/_ref: it holds reference object code).
set -euo pipefail
HERE="$(cd "$(dirname "$0")" && pwd)"
ROOT="$(dirname "$(dirname "$HERE")")"
REFOUT="$ROOT/oracle/_ref"
FC="${FC:-/opt/rocm/bin/amdflang}"
MKLDIR="${MKLDIR:-/opt/conda/lib}"
[ -f "$REFOUT/librslmto_ref.a" ] || { echo "oracle/_ref/librslmto_ref.a missing: run __graft_entry__.build() first" >&2; exit 1; }
mkdir -p "$REFOUT/moment_fixture"
cd "$REFOUT/moment_fixture"
"$FC" -cpp -O2 -fopenmp -I"$REFOUT/mod" -c "$HERE/moment_driver.f90" -o moment_driver.o
"$FC" moment_driver.o "$REFOUT/librslmto_ref.a" -fopenmp -L"$MKLDIR" -lmkl_rt -Wl,-rpath,"$MKLDIR" -o "$REFOUT/moment_driver.x"
echo "built $REFOUT/moment_driver.x"
