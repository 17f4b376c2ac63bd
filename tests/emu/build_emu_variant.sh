#!/bin/bash
# TEST INFRASTRUCTURE: host build of an fp32 variant of the unmodified kernel sources, like build_emu.sh.
#   build_emu_variant.sh [f32a]  the fp32-arithmetic variant (-DPOMGPU_STORE_F32 -DPOMGPU_COMPUTE_F32, libpomgpu_f32a.so's
#                                flags) into tests/_emu_f32a/libpomgpu_emu_f32a.so
#   build_emu_variant.sh f32     the fp32-storage variant (-DPOMGPU_STORE_F32, libpomgpu_f32.so's flags) into
#                                tests/_emu_f32/libpomgpu_emu_f32.so
set -euo pipefail
HERE=$(cd "$(dirname "$0")" && pwd); ROOT=$(cd "$HERE/../.." && pwd)
VARIANT=${1:-f32a}
case "$VARIANT" in
  f32a) DEFS="-DPOMGPU_STORE_F32 -DPOMGPU_COMPUTE_F32" ;;
  f32)  DEFS="-DPOMGPU_STORE_F32" ;;
  *) echo "usage: $0 [f32a|f32]" >&2; exit 2 ;;
esac
OUT=$ROOT/tests/_emu_$VARIANT; mkdir -p "$OUT"
SRC=$ROOT/extpom_amd/csrc
pids=()
FLAGS="-x c++ -std=c++17 -O2 -ffp-contract=off -fno-fast-math -fPIC -w $DEFS -I$HERE -I$ROOT/include -I$SRC"
for f in k_ext k_adv k_vert k_tile k_bc pomgpu_api transport cdf_out; do
  g++ $FLAGS -DPOMGPU_FILE_UNITS -c "$SRC/$f.hip" -o "$OUT/$f.o" & pids+=($!)
done
mkdir -p "$OUT/readers"   # the reader units of the file unit, apart from the objects a list without them links (cdf_out.hip's last lines)
for f in cdf_in frc_files ztosig; do
  g++ $FLAGS -c "$SRC/$f.hip" -o "$OUT/readers/$f.o" & pids+=($!)
done
g++ $FLAGS -c "$HERE/emu_support.cpp" -o "$OUT/emu_support.o" & pids+=($!)
for p in "${pids[@]}"; do wait "$p"; done     # a failed compile fails the build (plain `wait` would hide it)
g++ -shared -o "$OUT/libpomgpu_emu_$VARIANT.so" "$OUT"/*.o "$OUT"/readers/*.o -lm
echo "built $OUT/libpomgpu_emu_$VARIANT.so"
