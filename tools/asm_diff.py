#!/usr/bin/env python3
"""Is the device code of the named translation units the same in two source trees?

    python tools/asm_diff.py OLD_TREE NEW_TREE --units gemm gemm2 gemm_stagger [--keep DIR]

Compiles ucf-vit_amd/csrc/<unit>.hip of both trees to gfx950 assembly (device side only; the Makefile's common flags plus
the `FLAGS_<unit>` line of each tree's own Makefile, e.g. -ffp-contract=off for patcher_labels, the MFMA form for attention) and compares,
kernel by kernel, the instruction stream and the .amdhsa_* resource directives (VGPR / AGPR / SGPR counts, LDS size, scratch size).
What a pure move of code between files legitimately changes is normalised away: the index of the function in the numbers of local
labels, comments, .file / .ident / .loc directives and the order of the kernels in the file (a device-only compilation spells an
anonymous namespace _GLOBAL__N_1, without a per-file hash, so kernel names compare as they are).  Prints one verdict per
kernel; the exit status is 1 if a kernel is missing, extra or different, else 0.  Needs hipcc (HIPCC, default /opt/rocm/bin/hipcc), no GPU.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=fast", "--cuda-device-only", "-S"]
LABEL = re.compile(r"\.L(BB|func_begin|func_end|tmp|JTI)\d+(_\d+)?")


def unit_flags(tree, unit):
    """the unit's own flags: the tree's Makefile line `FLAGS_<unit> := ...`, which the build rule puts behind the common ones"""
    for line in open(os.path.join(tree, "ucf-vit_amd", "Makefile")):
        m = re.match(rf"FLAGS_{re.escape(unit)}\s*:?=\s*(.*)", line)
        if m:
            return m.group(1).split()
    return []


def compile_unit(tree, unit, out):
    src = os.path.join(tree, "ucf-vit_amd", "csrc", unit + ".hip")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc] + FLAGS + unit_flags(tree, unit) + ["-o", out, src], check=True, stderr=subprocess.DEVNULL)
    return out


def normalise(line):
    line = line.split(";", 1)[0].rstrip()
    # local labels: keep the block number inside the function, drop the function's index in the file
    return LABEL.sub(lambda m: ".L" + m.group(1) + (m.group(2) or ""), line)


def kernels(path):
    """name -> (instruction lines, .amdhsa_ lines)"""
    lines = [normalise(l) for l in open(path)]
    names = [l.split()[1] for l in lines if l.strip().startswith(".amdhsa_kernel ")]
    out = {}
    for name in names:
        start = lines.index(name + ":")
        end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
        body = [l.strip() for l in lines[start + 1:end] if l.strip() and not re.match(r"\s*\.(loc|file|ident|cfi_\w+)\b", l)]
        k0 = next(i for i, l in enumerate(lines) if l.strip() == ".amdhsa_kernel " + name)
        k1 = next(i for i in range(k0, len(lines)) if lines[i].strip() == ".end_amdhsa_kernel")
        out[name] = (body, [l.strip() for l in lines[k0 + 1:k1]])
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("old_tree")
    ap.add_argument("new_tree")
    ap.add_argument("--units", nargs="+", required=True, help="names of ucf-vit_amd/csrc/<unit>.hip")
    ap.add_argument("--keep", help="directory that receives the .s files (default: a temporary one)")
    a = ap.parse_args()
    tmp = a.keep or tempfile.mkdtemp(prefix="asm_diff_")
    os.makedirs(tmp, exist_ok=True)
    jobs = [(t, u, os.path.join(tmp, f"{side}_{u}.s")) for side, t in (("old", a.old_tree), ("new", a.new_tree)) for u in a.units]
    with ThreadPoolExecutor(max_workers=min(len(jobs), os.cpu_count() or 1, 8)) as ex:
        list(ex.map(lambda j: compile_unit(*j), jobs))
    bad = 0
    for u in a.units:
        old, new = kernels(os.path.join(tmp, f"old_{u}.s")), kernels(os.path.join(tmp, f"new_{u}.s"))
        for name in sorted(set(old) | set(new)):
            if name not in new or name not in old:
                verdict = "MISSING in the new tree" if name in old else "EXTRA in the new tree"
            elif old[name] == new[name]:
                verdict = f"identical ({len(new[name][0])} lines, {len(new[name][1])} directives)"
            else:
                (ob, od), (nb, nd) = old[name], new[name]
                first = next((i for i, (x, y) in enumerate(zip(ob, nb)) if x != y), min(len(ob), len(nb)))
                dirs = [f"{x} -> {y}" for x, y in zip(od, nd) if x != y]
                verdict = f"DIFFERENT (instructions {len(ob)} -> {len(nb)}, first difference at line {first}; directives: {dirs or 'same'})"
            bad += not verdict.startswith("identical")
            print(f"{u}: {name}: {verdict}")
        print(f"{u}: {len(old)} kernels in the old tree, {len(new)} in the new one")
    print("RESULT:", "device code identical" if not bad else f"{bad} kernels differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
