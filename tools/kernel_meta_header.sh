#!/bin/bash
# Register / scratch / spill figures of the kernels of one header of csrc/ from the code-object metadata (DESIGN.md 7h, 7j,
# 7k, 7l): a one-line file that includes the header, compiled to assembly for the device only.  With KEEP_ASM=file the
# listing is kept there (tools/isa_loops.py reads it).
#   tools/kernel_meta_header.sh <header, e.g. simulate.h> <kernel-name pattern, e.g. k_sim> [extra hipcc flags]
[ $# -ge 2 ] || { echo "usage: $0 <header> <kernel-name pattern> [hipcc flags]" >&2; exit 2; }
HDR=$1; PAT=$2; shift 2
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
python3 "$ROOT/altro-mpc-icra2021_amd/csrc/gen_dpp_blocks.py" "$ROOT/altro-mpc-icra2021_amd/csrc/dpp_blocks.inc"
T=$(mktemp -d)
echo "#include \"$ROOT/altro-mpc-icra2021_amd/csrc/$HDR\"" > $T/one.hip
hipcc --offload-arch=gfx950 -O3 -std=c++17 -S --cuda-device-only -Wno-unused-value "$@" -o $T/one.s $T/one.hip || exit 1
grep -E "^\s+\.(name|vgpr_count|sgpr_count|agpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size):" $T/one.s |
  tr -s ' ' | awk '/\.name:/ { if (line) print line; line = $2; next } { line = line " " $1 " " $2 } END { print line }' | grep -E "$PAT"
[ -n "$KEEP_ASM" ] && cp $T/one.s "$KEEP_ASM"
rm -rf $T
