#!/bin/bash
# Register / scratch / spill figures of the two kernels of csrc/simulate.h from the code-object metadata.
#   tools/kernel_meta_simulate.sh [extra hipcc flags]
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
python3 "$ROOT/altro-mpc-icra2021_amd/csrc/gen_dpp_blocks.py" "$ROOT/altro-mpc-icra2021_amd/csrc/dpp_blocks.inc"
T=$(mktemp -d)
echo "#include \"$ROOT/altro-mpc-icra2021_amd/csrc/simulate.h\"" > $T/one.hip
hipcc --offload-arch=gfx950 -O3 -std=c++17 -S --cuda-device-only -Wno-unused-value "$@" -o $T/one.s $T/one.hip || exit 1
grep -E "^\s+\.(name|vgpr_count|sgpr_count|agpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size):" $T/one.s |
  tr -s ' ' | awk '/\.name:/ { if (line) print line; line = $2; next } { line = line " " $1 " " $2 } END { print line }' | grep k_sim
rm -rf $T
