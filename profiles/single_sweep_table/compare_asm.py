#!/usr/bin/env python
"""Device assembly of two builds, kernel by kernel:  compare_asm.py PARENT_DIR BRANCH_DIR

Each directory holds one `<unit>.s` per translation unit, written by hipcc with the build's flags (tidy3d_amd/build.py) plus
`--offload-device-only -S`.  A kernel's text is everything between its label and its `.Lfunc_end` (instructions and the
`.amdhsa_kernel` block: registers, scratch, LDS); its entry of the `amdhsa.kernels` metadata is compared too.  Masked: the
`__hip_cuid_*` symbol, the function's number inside local labels (`.LBB<n>_<m>`) and comments.  The instantiations of
`fused_step_kernel` (fdtd_capi.hip) are reported one by one, every other kernel per unit."""
import glob
import os
import re
import subprocess
import sys

SWEEP = "fused_step_kernelILb"
META = ("agpr_count", "group_segment_fixed_size", "kernarg_segment_size", "max_flat_workgroup_size", "private_segment_fixed_size",
        "sgpr_count", "sgpr_spill_count", "vgpr_count", "vgpr_spill_count", "uses_dynamic_stack", "wavefront_size")


def norm_body(lines):
    text = "".join(re.sub(r"\s*;.*$", "", ln.rstrip()) + "\n" for ln in lines)
    text = re.sub(r"__hip_cuid_\w+", "__hip_cuid_X", text)
    return re.sub(r"\.L(BB|JTI|CPI)\d+_", r".L\1N_", text)


def kernels(path):
    """name -> (normalised text, metadata fields)"""
    body, meta, name, cur, entry = {}, {}, None, [], None
    for line in open(path):
        m = re.match(r"^(_Z\w+):\s", line)
        if m and name is None:
            name, cur = m.group(1), []
        elif name is not None:
            if line.startswith(".Lfunc_end"):
                body[name] = norm_body(cur)
                name = None
            else:
                cur.append(line)
        if line.startswith("  - .agpr_count:"):
            entry = {}
        m = re.match(r"^  [ -] \.(\w+):\s+(\S+)", line)
        if m and entry is not None:
            entry[m.group(1)] = m.group(2)
            if m.group(1) == "wavefront_size":
                meta[entry["name"]] = tuple(entry.get(k) for k in META)
                entry = None
    return {k: (body[k], meta[k]) for k in body if k in meta}       # (kernels only: device functions have no metadata entry)


def demangle(n):
    return subprocess.run(["c++filt", n], capture_output=True, text=True).stdout.strip().split("(")[0]


def line(n, k):
    f = dict(zip(META, k[1]))
    n_ins = sum(1 for ln in k[0].splitlines() if re.match(r"^\s+[a-z]\w+", ln))       # (directives start with a dot)
    return (f"  {demangle(n)[-60:]:60s} vgpr {f['vgpr_count']:>3s} sgpr {f['sgpr_count']:>3s} scratch {f['private_segment_fixed_size']:>3s} "
            f"spills s/v {f['sgpr_spill_count']}/{f['vgpr_spill_count']} lds {f['group_segment_fixed_size']} instructions {n_ins}")


parent, branch = sys.argv[1], sys.argv[2]
A = {os.path.basename(p): kernels(p) for p in sorted(glob.glob(os.path.join(parent, "*.s")))}
B = {os.path.basename(p): kernels(p) for p in sorted(glob.glob(os.path.join(branch, "*.s")))}
bad = 0
sweep_a = {k: v for k, v in A["fdtd_capi.s"].items() if SWEEP in k}
sweep_b = {k: v for k, v in B["fdtd_capi.s"].items() if SWEEP in k}
print("Device code for gfx950, parent against branch (labels renumbered, comments dropped; instructions, .amdhsa_kernel block and")
print("metadata: " + ", ".join(META) + ")")
print(f"\nfused_step_kernel: {len(sweep_a)} instantiations in the parent's fdtd_capi.hip, {len(sweep_b)} in the branch's, "
      f"{sum(1 for u, ks in B.items() if u != 'fdtd_capi.s' for k in ks if SWEEP in k)} in the branch's other units")
same = [k for k in sweep_b if k in sweep_a and sweep_a[k] == sweep_b[k]]
differ = [k for k in sweep_b if k in sweep_a and sweep_a[k] != sweep_b[k]]
new = [k for k in sweep_b if k not in sweep_a]
gone = [k for k in sweep_a if k not in sweep_b]
bad += len(differ) + len(new)
print(f"  identical to the parent's copy, instruction for instruction and in every metadata field: {len(same)}")
print(f"  differ: {len(differ)}   new: {len(new)}   gone from the library: {len(gone)}")
for title, ks, src in (("differ", differ, sweep_b), ("new", new, sweep_b), ("gone from the library (the dead instantiations)", gone, sweep_a), ("identical", same, sweep_b)):
    if ks:
        print(title + ":")
        for k in sorted(ks, key=demangle):
            print(line(k, src[k]))
print()
for unit in A:
    a = {k: v for k, v in A[unit].items() if SWEEP not in k}
    b = {k: v for k, v in B.get(unit, {}).items() if SWEEP not in k}
    d = [k for k in a if k in b and a[k] != b[k]]
    g = [k for k in a if k not in b]
    n = [k for k in b if k not in a]
    bad += len(d) + len(g) + len(n)
    print(f"{unit[:-2]}.hip: {len(a)} other kernels in the parent, {len(b)} in the branch: {len(a) - len(d) - len(g)} identical, {len(d)} differ, {len(g)} missing, {len(n)} new")
    for tag, ks in (("DIFFERS", d), ("MISSING", g), ("NEW", n)):
        for k in ks:
            print(f"  {tag} {demangle(k)}")
sys.exit(1 if bad else 0)
