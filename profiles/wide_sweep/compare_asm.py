#!/usr/bin/env python
"""Device assembly of two builds, kernel by kernel:  compare_asm.py PARENT_DIR BRANCH_DIR

Each directory holds one `<unit>.s` per translation unit, written by hipcc with the build's flags (tidy3d_amd/build.py) plus
`--offload-device-only -S`.  A kernel's text is everything between its label and its `.Lfunc_end`; the `__hip_cuid_*` symbol differs
between any two compilations and is masked, and so is the function's number inside its local labels (`.LBB<n>_<m>`); comments are dropped.  `fused_step_kernel` gained a trailing template parameter (WIDE, default false): the
branch's `..., false>` instantiations are compared under the parent's names, the `..., true>` ones are listed as new."""
import glob
import os
import re
import subprocess
import sys


def kernels(path):
    out, name, body = {}, None, []
    for line in open(path):
        m = re.match(r"^(_Z\w+):\s", line)
        if m and name is None:
            name, body = m.group(1), []
            continue
        if name is not None:
            if line.startswith(".Lfunc_end"):
                out[name] = body
                name = None
            else:
                body.append(line)
    return out


def norm_name(n):
    # fused_step_kernel<MAT, LB, PML, HINT, false>  ->  fused_step_kernel<MAT, LB, PML, HINT>
    return re.sub(r"(fused_step_kernelILb[01]ELi\d+ELi\d+ELi\d+E)Lb0E", r"\1", n)


def norm_body(lines):
    text = "".join(re.sub(r"\s*;.*$", "", ln.rstrip()) + "\n" for ln in lines)     # (comments name loop headers by function number)
    text = re.sub(r"__hip_cuid_\w+", "__hip_cuid_X", text)
    text = re.sub(r"\.L(BB|JTI|CPI)\d+_", r".L\1N_", text)        # local labels carry the function's number within its unit
    return re.sub(r"(fused_step_kernelILb[01]ELi\d+ELi\d+ELi\d+E)Lb0E", r"\1", text)


def demangle(n):
    return subprocess.run(["c++filt", n], capture_output=True, text=True).stdout.strip().split("(")[0]


parent, branch = sys.argv[1], sys.argv[2]
same = changed = 0
new, gone, diff = [], [], []
for p in sorted(glob.glob(os.path.join(parent, "*.s"))):
    unit = os.path.basename(p)
    a = {norm_name(k): norm_body(v) for k, v in kernels(p).items()}
    b = {norm_name(k): norm_body(v) for k, v in kernels(os.path.join(branch, unit)).items()}
    for k in a:
        if k not in b:
            gone.append((unit, k))
        elif a[k] == b[k]:
            same += 1
        else:
            changed += 1
            diff.append((unit, k))
    new += [(unit, k) for k in b if k not in a]
    print(f"{unit}: {len(a)} kernels in the parent, {len(b)} here")
print(f"identical: {same}   changed: {changed}   removed: {len(gone)}   new: {len(new)}")
for unit, k in diff:
    print(f"CHANGED {unit} {demangle(k)}")
for unit, k in gone:
    print(f"REMOVED {unit} {demangle(k)}")
for unit, k in new:
    print(f"new     {unit} {demangle(k)}")
sys.exit(1 if changed or gone else 0)
