#!/bin/bash
# Builds dbg/libdudf_<tag>.so with extra -D flags for EVERY translation unit:  bash tools/build_all_dbg.sh <tag> "-DDUDF_P24_ARRAYS=2"
R=$(cd "$(dirname "$0")/.." && pwd)
tag=$1; flags=$2
mkdir -p "$R/dbg/obj_$tag"
objs=""
# the translation units of the library: SRCS of csrc/Makefile
for src in $(sed -n 's/^SRCS *= *//p' "$R/diffudf_amd/csrc/Makefile"); do
  u=${src%.hip}
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC $flags -c "$R/diffudf_amd/csrc/$src" -o "$R/dbg/obj_$tag/$u.o" &
  objs="$objs $R/dbg/obj_$tag/$u.o"
done
wait
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o "$R/dbg/libdudf_$tag.so" $objs && rm -rf "$R/dbg/obj_$tag"
