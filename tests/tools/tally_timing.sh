#!/bin/bash
# The measurements of DESIGN.md 3.15 in one go, from the repository root on a machine with a GPU, the library and the programs
# built (and oracle/_ref/kaiju2table, for the last step):
#     bash tests/tools/tally_timing.sh [OUT_DIR] [MIB]
# Every step runs under a time limit of its own and the next one only starts when it succeeded.  What the steps print - one JSON
# line each, and the per-kernel statistics of the trace - lands in OUT_DIR (default: tally_timing_out).
set -o pipefail
OUT=${1:-tally_timing_out}
MIB=${2:-1024}
WORK=${TMPDIR:-/tmp}/kaiju_amd_tally_timing
mkdir -p "$OUT" "$WORK"
timeout -k 10 420 python tests/tools/tally_timing.py passes --work "$WORK" --mib "$MIB" 2> "$OUT/passes.err" | tee "$OUT/passes.json" &&
timeout -k 10 420 rocprofv3 --kernel-trace --stats -d "$WORK/trace" -o tally --output-format csv -- python tests/tools/tally_timing.py kernels --work "$WORK" --mib "$MIB" > "$OUT/kernels.json" 2> "$OUT/kernels.err" &&
{ find "$WORK/trace" -name '*kernel_stats.csv' -exec grep -E '^"?Name|k_an_|k_tl_' {} + | tee "$OUT/kernel_stats.csv"; } &&
timeout -k 10 600 python tests/tools/tally_timing.py cli --work "$WORK" --mib "$MIB" 2> "$OUT/cli.err" | tee "$OUT/cli.json"
rc=$?
rm -rf "$WORK"
exit $rc
