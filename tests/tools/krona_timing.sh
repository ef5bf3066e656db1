#!/bin/bash
# The measurements of DESIGN.md 3.16 in one go, from the repository root on a machine with a GPU, the library and the programs
# built (and oracle/_ref/kaiju2krona, for the second step):
#     bash tests/tools/krona_timing.sh [OUT_DIR] [MIB]
# Every step runs under a time limit of its own and the next one only starts when it succeeded.  What the steps print - one JSON
# line each - lands in OUT_DIR (default: krona_timing_out).
set -o pipefail
OUT=${1:-krona_timing_out}
MIB=${2:-1024}
WORK=${TMPDIR:-/tmp}/kaiju_amd_krona_timing
mkdir -p "$OUT" "$WORK"
timeout -k 10 300 python tests/tools/krona_timing.py passes --work "$WORK" --mib "$MIB" 2> "$OUT/passes.err" | tee "$OUT/passes.json" &&
timeout -k 10 600 python tests/tools/krona_timing.py cli --work "$WORK" --mib "$MIB" 2> "$OUT/cli.err" | tee "$OUT/cli.json"
rc=$?
rm -rf "$WORK"
exit $rc
