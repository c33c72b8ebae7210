#!/bin/bash
# Builds the exchange fixture driver against the compiled reference that build() leaves in oracle/_ref (librslmto_ref.a, mod/).
# Output: oracle/_ref/exchange_driver.x (git-ignored with the rest of oracle/_ref: it holds reference object code).
set -euo pipefail
HERE="$(cd "$(dirname "$0")" && pwd)"
ROOT="$(dirname "$(dirname "$HERE")")"
REFOUT="$ROOT/oracle/_ref"
FC="${FC:-/opt/rocm/bin/amdflang}"
MKLDIR="${MKLDIR:-/opt/conda/lib}"
[ -f "$REFOUT/librslmto_ref.a" ] || { echo "oracle/_ref/librslmto_ref.a missing: run __graft_entry__.build() first" >&2; exit 1; }
mkdir -p "$REFOUT/exchange_fixture"
cd "$REFOUT/exchange_fixture"
"$FC" -cpp -O2 -fopenmp -I"$REFOUT/mod" -c "$HERE/exchange_driver.f90" -o exchange_driver.o
"$FC" exchange_driver.o "$REFOUT/librslmto_ref.a" -fopenmp -L"$MKLDIR" -lmkl_rt -Wl,-rpath,"$MKLDIR" -o "$REFOUT/exchange_driver.x"
echo "built $REFOUT/exchange_driver.x"
