#!/usr/bin/env python3
"""Print VGPR / SGPR / scratch / occupancy / LDS per kernel from the device listings of `make asm` (the numbers the compiler
prints behind each function).  Usage: python tools/kernel_resources.py [substring filter]"""
import glob
import os
import re
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from isa_diff import read_listing

subprocess.run(["make", "-s", "-C", "fm-for-online-recommendation_amd/csrc", "asm"], check=True, capture_output=True)
flt = sys.argv[1] if len(sys.argv) > 1 else ""
for path in sorted(glob.glob("fm-for-online-recommendation_amd/csrc/build/asm/fmx_*.s")):
    for name, f in read_listing(path).items():
        k, v = re.sub(r"_ZN12_GLOBAL__N_1\d+", "", name), f["numbers"]
        if f["desc"] is not None and flt in k:
            print(f"{k[:48]:48s} VGPR={v.get('NumVgprs'):>4} SGPR={v.get('TotalNumSgprs'):>4} scratch={v.get('ScratchSize'):>3} "
                  f"occ={v.get('Occupancy')} LDS={v.get('LDSByteSize')}")
