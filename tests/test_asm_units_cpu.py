"""`make asm` (csrc/Makefile) lists every unit whose kernels tools/isa_diff.py and tools/kernel_resources.py are asked about: the
table kernels' units and the mini-batch MLP's (fmx_mlp: k_mlp_chain, k_mlp_loss, k_mlp_pair_loss, the GEMMs).  A dry run: nothing is
compiled."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fm-for-online-recommendation_amd", "csrc")


def test_make_asm_lists_the_mlp_unit_beside_the_table_units(tmp_path):
    out = subprocess.run(["make", "-n", "-C", CSRC, "asm", f"ASMD={tmp_path}"], capture_output=True, text=True, check=True).stdout
    listed = set(re.findall(r"-o\s+" + re.escape(str(tmp_path)) + r"/(\w+)\.s\s+(?:\S*/)?(\w+)\.hip", out))
    units = {unit for unit, src in listed}
    assert all(unit == src for unit, src in listed), listed                      # each listing comes from its own unit
    assert "fmx_mlp" in units, f"`make asm` does not list the MLP unit: {sorted(units)}"
    assert {"fmx_kernels", "fmx_update", "fmx_online", "fmx_topk", "fmx_afm", "fmx_afm_pair_online", "fmx_list_online"} <= units
    # the listing is a device-only one with the compiler's resource remarks, which tools/isa_diff.read_listing parses
    line = next(ln for ln in out.splitlines() if "fmx_mlp.hip" in ln or "fmx_mlp.s" in ln)
    assert "--cuda-device-only" in out and "-S" in line.split() and "kernel-resource-usage" in out
    # every unit that holds kernels of the library's hot paths and is built into libfmx.so is either listed or known not to be
    built = set(re.search(r"^UNITS\s*:=\s*(.*)$", open(os.path.join(CSRC, "Makefile")).read(), re.M).group(1).split())
    assert units <= built and built - units == {"fmx_sftrl", "fmx_comm"}, (sorted(built - units), sorted(units - built))
