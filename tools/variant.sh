#!/bin/bash
# tools/variant.sh NAME [-DFLAG=VALUE ...] -- build sampler_amd/csrc/variants/NAME.so, a copy of
# libdwx.so compiled with extra flags (kernel A/B experiments).  Use it with DWX_LIB=<path>.
set -e
cd "$(dirname "$0")/../sampler_amd/csrc"
name=$1; shift
mkdir -p variants
/opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -Wall -Wno-unused-function \
  "$@" -x hip -c -o variants/$name.o dwx_api.cc
# (the graph compiler shares device_types.h with the kernels: same flags)
g++ -O2 -std=c++17 -fPIC -Wall -Wextra -pthread "$@" -c -o variants/$name.gc.o graph_compile.cc
# (the plan-level host builders share device_types.h too, so the defines reach them: the Makefile's flags of level_build.o)
g++ -O3 -std=c++17 -fPIC -Wall -Wextra -pthread -ffp-contract=off "$@" -c -o variants/$name.lb.o level_build.cc
# (... and so does the device builder: it packs the sorted records' owner field, DWX_SORT_OWNER_BITS)
/opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -Wall -Wno-unused-function \
  "$@" -c -o variants/$name.db.o device_build.hip
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o variants/$name.so variants/$name.o variants/$name.gc.o variants/$name.lb.o variants/$name.db.o -pthread
rm -f variants/$name.o variants/$name.gc.o variants/$name.lb.o variants/$name.db.o
echo "built sampler_amd/csrc/variants/$name.so"
