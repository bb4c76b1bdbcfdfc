#!/bin/bash
# Diagnostic build of the FM unit with in-kernel stamps (-DFMX_STAMPS) into tools/micro/libfmx_stamps.so, and the report.  Run the BUILD
# here (hipcc cross-compiles), the report on the GPU box:  bash tools/update_stamps.sh build ;  gpurun -- bash tools/update_stamps.sh run
set -e
root=$(cd "$(dirname "$0")/.." && pwd)
csrc=$root/fm-for-online-recommendation_amd/csrc
if [ "$1" = "build" ]; then
  make -s -j4 -C $csrc
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -I$root/include -I/opt/rocm/include -DFMX_STAMPS -c -o /tmp/fmx_kernels_stamps.o $csrc/fmx_kernels.hip
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $root/tools/micro/libfmx_stamps.so /tmp/fmx_kernels_stamps.o $csrc/build/fmx_mlp.o $csrc/build/fmx_sftrl.o $csrc/build/fmx_comm.o $csrc/build/fmx_topk.o $csrc/build/fmx_afm.o -ldl
else
  FMX_LIB_PATH=$root/tools/micro/libfmx_stamps.so python3 $root/tools/update_stamps.py
fi
