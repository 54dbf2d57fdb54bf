#!/bin/bash
# Builds dbg/libdudf_<tag>.so with extra -D flags for ONE translation unit, or for a few (debug builds):
#   bash tools/build_dbg.sh <tag> <unit: sweep_bf16|sweep_wide|prep|wgrad|...> "-DDUDF_LATE_FORCE=1"
#   bash tools/build_dbg.sh <tag> "sweep_bf16 sweep_wide" "-DDUDF_FX_CHECK=1"
# The other units are the objects of the regular build (make -C diffudf_amd/csrc).
R=$(cd "$(dirname "$0")/.." && pwd)
tag=$1; units=$2; flags=$3
mkdir -p "$R/dbg"
B=$R/diffudf_amd/csrc/build
for unit in $units; do
  rm -f "$R/dbg/${unit}_$tag.o"
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC $flags -c "$R/diffudf_amd/csrc/dudf_$unit.hip" -o "$R/dbg/${unit}_$tag.o" &
done
wait
objs=""
# the translation units of the library: SRCS of csrc/Makefile
for src in $(sed -n 's/^SRCS *= *//p' "$R/diffudf_amd/csrc/Makefile"); do
  u=${src%.hip}; u=${u#dudf_}
  case " $units " in
    *" $u "*) [ -f "$R/dbg/${u}_$tag.o" ] || exit 1; objs="$objs $R/dbg/${u}_$tag.o";;
    *) objs="$objs $B/dudf_$u.o";;
  esac
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o "$R/dbg/libdudf_$tag.so" $objs
