#!/bin/bash
# tools/build_variant.sh NAME -DMACRO=V ...  -> variants/libggmres_NAME.so
# (kernels.hip and every file under csrc/kernels/ rebuilt with the given macros, in
# parallel -- the GG_WAVE_* / GG_TILE_* macros reach kernels/trsv_wave.hip,
# GG_WAVE_SUM_SHFL the shared kernels/device.h -- other objects from the main build;
# select at run time with GGMRES_LIB=variants/libggmres_NAME.so; VARDIR=abvar puts
# it in abvar/ instead, which travels to the GPU box -- variants/ does not)
set -e
cd "$(dirname "$0")/../gpu-gmres_amd"
name=$1; shift
VD=${VARDIR:-variants}
mkdir -p ../$VD build/var/$name
pids=()
for f in csrc/kernels.hip csrc/kernels/*.hip; do
    /opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC -ffp-contract=off --offload-arch=gfx950 -I../include/compat -I../include -Icsrc \
        "$@" -c $f -o build/var/$name/$(basename $f .hip).o &
    pids+=($!)
done
for p in "${pids[@]}"; do wait $p; done
/opt/rocm/bin/hipcc -shared --offload-arch=gfx950 -o ../$VD/libggmres_$name.so build/var/$name/*.o \
    $(find build -name "*.o" ! -path "build/var/*" ! -path "build/kernels/*" ! -name kernels.o | sort) -L/opt/rocm/lib -lamdhip64 -lrccl -Wl,-rpath,/opt/rocm/lib
