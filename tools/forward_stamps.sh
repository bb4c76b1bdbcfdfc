#!/bin/bash
# In-kernel stamps of k_fm_forward (-DFMX_STAMPS: the diagnostic library tools/update_stamps.sh builds into tools/micro/libfmx_stamps.so)
# and the report.  The build needs only hipcc (it cross-compiles); the report runs on the MI355X:
#   bash tools/forward_stamps.sh build ;  bash tools/forward_stamps.sh run
set -e
root=$(cd "$(dirname "$0")/.." && pwd)
if [ "$1" = "build" ]; then
  bash $root/tools/update_stamps.sh build
else
  FMX_LIB_PATH=${FMX_LIB_PATH:-$root/tools/micro/libfmx_stamps.so} python3 $root/tools/forward_stamps.py
fi
