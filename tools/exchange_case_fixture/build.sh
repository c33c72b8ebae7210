#!/bin/bash
# Builds the case dump of the drop-in exchange fixtures against the compiled reference that build() leaves in oracle/_ref
# (librslmto_ref.a, mod/), and the per-pair exchange driver of tools/exchange_fixture.  Outputs (git-ignored with the rest of
# oracle/_ref: they hold reference object code): oracle/_ref/exchange_case_dump.x, oracle/_ref/exchange_driver.x
set -euo pipefail
HERE="$(cd "$(dirname "$0")" && pwd)"
ROOT="$(dirname "$(dirname "$HERE")")"
REFOUT="$ROOT/oracle/_ref"
FC="${FC:-/opt/rocm/bin/amdflang}"
MKLDIR="${MKLDIR:-/opt/conda/lib}"
[ -f "$REFOUT/librslmto_ref.a" ] || { echo "oracle/_ref/librslmto_ref.a missing: run __graft_entry__.build() first" >&2; exit 1; }
bash "$ROOT/tools/exchange_fixture/build.sh"
mkdir -p "$REFOUT/exchange_case_fixture"
cd "$REFOUT/exchange_case_fixture"
"$FC" -cpp -O2 -fopenmp -I"$REFOUT/mod" -c "$HERE/case_dump.f90" -o case_dump.o
"$FC" case_dump.o "$REFOUT/librslmto_ref.a" -fopenmp -L"$MKLDIR" -lmkl_rt -Wl,-rpath,"$MKLDIR" -o "$REFOUT/exchange_case_dump.x"
echo "built $REFOUT/exchange_case_dump.x"
