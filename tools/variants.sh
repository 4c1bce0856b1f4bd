#!/bin/bash
# tools/variants.sh NAME "-DFLAG1 -DFLAG2"   → builds optixpathtracer_amd/variants/libptamd_NAME.so (A/B experiments)
set -e
NAME=$1; DEFS=$2
cd "$(dirname "$0")/../optixpathtracer_amd/csrc"
mkdir -p ../variants
FLAGS="-O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off -fno-slp-vectorize -fPIC -Wno-unused-result -Wno-unused-value $DEFS"
# objects next to the library (inside the tree, not in a shared temporary directory); each compile's status is checked
/opt/rocm/bin/hipcc $FLAGS -c pt_lib.hip -o ../variants/pt_api_$NAME.o & P1=$!
/opt/rocm/bin/hipcc $FLAGS -c pt_bvh_build.hip -o ../variants/pt_bvh_build_$NAME.o & P2=$!
wait $P1
wait $P2
make -s pt_objload.o  # the host-only scene ingestion is the same in every variant
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o ../variants/libptamd_$NAME.so ../variants/pt_api_$NAME.o ../variants/pt_bvh_build_$NAME.o pt_objload.o -ldl
echo built variants/libptamd_$NAME.so
