#!/usr/bin/env python3
"""Compare two directories of device-only assembly listings (`make -C .../csrc asm ASMD=<dir>` at two commits), kernel by kernel.

    python tools/isa_diff.py <dir_before> <dir_after> [-v]

Every function of every *.s file is taken apart: its instruction text (comments dropped; the function number in local labels and
the per-unit hash that internal-linkage symbols carry normalised away), and for kernels the kernel descriptor and the
VGPR / SGPR / LDS / scratch numbers the compiler prints behind the function.  Kernels and device functions are matched by name over
the whole directory, so a kernel that moved to another translation unit is compared with itself.  Prints what differs, what is
missing, what is new and what appears more than once, then one summary line; the exit status is 0 only if nothing differs and
nothing is missing.  The comparison is textual: it knows nothing about particular instructions."""
import collections
import glob
import os
import re
import shutil
import subprocess
import sys

HASH = re.compile(r"(\.intern\.|__intern__|\.static\.|__static__)[0-9a-f]{6,}")
LOCAL = re.compile(r"\.L(BB|JTI|func_begin|func_end|tmp)\d+")
NUMBERS = ("TotalNumSgprs", "NumVgprs", "NumAgprs", "TotalNumVgprs", "ScratchSize", "LDSByteSize", "Occupancy", "codeLenInByte")


def norm(line):
    line = line.split(";", 1)[0].rstrip()
    return LOCAL.sub(lambda m: ".L" + m.group(1), HASH.sub("", line))


def read_listing(path):
    """{name: dict(text=[...], desc=[...] or None, numbers={...}, unit=...)} of one listing"""
    out, cur, desc = {}, None, None
    unit = os.path.basename(path)
    for raw in open(path, errors="replace"):
        raw = raw.rstrip("\n")
        m = re.match(r"^([A-Za-z_$][\w$.]*):", raw)
        if m and cur is None and "@function" not in raw and not raw.startswith(".L"):
            if re.search(r";\s*@", raw):  # a function's entry label carries "; @name"
                cur = HASH.sub("", m.group(1))
                out[cur] = dict(text=[], desc=None, numbers={}, unit=unit)
                continue
        s = raw.strip()
        if s.startswith(".amdhsa_kernel "):
            desc = HASH.sub("", s.split()[1])
            out.setdefault(desc, dict(text=[], desc=None, numbers={}, unit=unit))["desc"] = []
            continue
        if s == ".end_amdhsa_kernel":
            desc = None
            continue
        if desc is not None:
            out[desc]["desc"].append(norm(s))
            continue
        if cur is None:
            continue
        if re.match(r"^\.Lfunc_end\d+:", s):
            cur = None
            continue
        if s and not s.startswith(";"):
            t = norm(raw)
            if t.strip():
                out[cur]["text"].append(t)
    # the "; NumVgprs: 15" block behind each function
    cur = None
    for raw in open(path, errors="replace"):
        m = re.match(r"^([A-Za-z_$][\w$.]*):.*;\s*@", raw)
        if m:
            cur = HASH.sub("", m.group(1))
        m = re.match(r"^;\s*(\w+)\s*[:=]\s*(\d+)", raw)
        if m and cur in out and m.group(1) in NUMBERS:
            out[cur]["numbers"][m.group(1)] = int(m.group(2))
    return out


def read_dir(d):
    fns = collections.defaultdict(list)
    for path in sorted(glob.glob(os.path.join(d, "*.s"))):
        for name, f in read_listing(path).items():
            fns[name].append(f)
    return fns


def demangle(names):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt") or "/opt/rocm/llvm/bin/llvm-cxxfilt"
    try:
        res = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
        return dict(zip(names, res))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def main(argv):
    verbose = "-v" in argv
    dirs = [a for a in argv if not a.startswith("-")]
    if len(dirs) != 2:
        sys.exit(__doc__)
    a, b = read_dir(dirs[0]), read_dir(dirs[1])
    pretty = demangle(sorted(set(a) | set(b)))
    count = collections.Counter()
    for name in sorted(set(a) | set(b), key=lambda n: pretty[n]):
        fa, fb = a.get(name, []), b.get(name, [])
        kind = "kernel" if any(f["desc"] is not None for f in fa + fb) else "function"
        where = lambda fs: ",".join(f["unit"] for f in fs)
        if not fb:
            count[kind, "missing"] += 1
            print(f"MISSING {kind} {pretty[name]}  (was in {where(fa)})")
        elif not fa:
            count[kind, "new"] += 1
            print(f"NEW     {kind} {pretty[name]}  (in {where(fb)})")
        elif len(fa) != 1 or len(fb) != 1:
            count[kind, "repeated"] += 1
            print(f"REPEATED {kind} {pretty[name]}  ({where(fa)} -> {where(fb)})")
        else:
            x, y = fa[0], fb[0]
            what = [w for w, same in (("instructions", x["text"] == y["text"]), ("descriptor", x["desc"] == y["desc"]),
                                      ("numbers", x["numbers"] == y["numbers"])) if not same]
            if what:
                count[kind, "differ"] += 1
                print(f"DIFFERS {kind} {pretty[name]}  ({x['unit']} -> {y['unit']}): {', '.join(what)}")
                if "numbers" in what:
                    print(f"        {x['numbers']}\n     -> {y['numbers']}")
                if "instructions" in what:
                    print(f"        {len(x['text'])} -> {len(y['text'])} lines")
            else:
                count[kind, "identical"] += 1
                if verbose:
                    print(f"same    {kind} {pretty[name]}  ({x['unit']} -> {y['unit']})")
    parts = []
    for kind in ("kernel", "function"):
        parts.append(f"{kind}s: " + ", ".join(f"{count[kind, k]} {k}" for k in ("identical", "differ", "missing", "new", "repeated")))
    print("isa_diff: " + "; ".join(parts))
    bad = sum(v for (kind, k), v in count.items() if k in ("differ", "missing", "repeated"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
