#!/bin/bash
# Build libtgis_hip.so for gfx950 in-tree (the .so travels to the GPU box with the snapshot).
# The units listed in tools/preload_units.txt are compiled with kernarg preload (leading scalar kernel parameters arrive
# in SGPRs at wave launch, csrc/gptq_wide_body.h), the others without: as __graft_entry__.build() does.
# Extra arguments go to every compile.  TGIS_LIB_SUFFIX=_ring16 tools/build.sh -DTGIS_MOE_GPTQ_RING=16 builds a variant,
# lib/libtgis_hip_ring16.so with its objects under lib/obj_ring16, beside the default library (tools/bench_mixtral.py --ring).
set -e
TOOLS="$(cd "$(dirname "$0")" && pwd)"
cd "$TOOLS/../text-generation-inference_amd"
SUFFIX="${TGIS_LIB_SUFFIX:-}"
OBJ="lib/obj$SUFFIX"
mkdir -p "$OBJ"
objs=()
pids=()
for src in csrc/*.hip; do
    unit=$(basename "$src")
    pre=()
    if grep -qx "$unit" "$TOOLS/preload_units.txt"; then pre=(-mllvm -amdgpu-kernarg-preload-count=16); fi
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC "${pre[@]}" "$@" -c "$src" -o "$OBJ/${unit%.hip}.o" &
    pids+=($!)
    objs+=("$OBJ/${unit%.hip}.o")
done
for p in "${pids[@]}"; do wait "$p"; done  # (set -e: a failed compile ends the build)
hipcc --offload-arch=gfx950 -shared -fPIC -o "lib/libtgis_hip$SUFFIX.so" "${objs[@]}"
