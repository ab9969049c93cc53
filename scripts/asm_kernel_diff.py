"""Compare the device code of two ``hipcc --cuda-device-only -S`` outputs kernel by kernel.

    python scripts/asm_kernel_diff.py OLD.s NEW.s [--table]

Per kernel symbol: the instruction stream (labels, comments, debug and line directives
dropped) and the ``.amdhsa_*`` resource block (VGPRs, SGPRs, LDS, scratch).  Symbol order
and line metadata may differ; anything else is reported.  Exit status 1 on a difference.
--table: one markdown row per differing kernel instead, old / new of ``next_free_vgpr``,
``next_free_sgpr``, scratch bytes, LDS bytes, occupancy and the instruction count.
"""
from __future__ import annotations

import re
import subprocess
import sys

_SKIP = re.compile(
    r"^\s*(\.loc|\.file|\.cfi_|\.Ltmp|\.Lfunc_|;|\.p2align|\.section|\.text|\.ident)")


def kernels(path):
    out, name, body = {}, None, []
    for line in open(path, errors="replace"):
        if line.lstrip().startswith(".amdgpu_metadata"):  # (the YAML repeats the blocks above)
            break
        m = re.match(r"^([A-Za-z_][\w$.]*):\s*(;.*)?$", line)
        if m and not m.group(1).startswith((".L", "__hip_cuid_")):
            name, body = m.group(1), []
            out[name] = body
            continue
        if name is None or _SKIP.match(line) or not line.strip() or "__hip_cuid_" in line:
            continue  # (__hip_cuid_*: the compilation unit's id, a hash of the source)
        body.append(line.split(";")[0].rstrip())
    return out


_RES = ("next_free_vgpr", "next_free_sgpr", "private_segment_fixed_size",
        "group_segment_fixed_size")


def resources(path, body):
    """symbol -> [vgpr, sgpr, scratch, lds, occupancy, instructions]"""
    out = {}
    for k, lines in body.items():
        r = dict.fromkeys(_RES, 0)
        for ln in lines:
            m = re.match(r"\s*\.amdhsa_(\w+)\s+(\d+)", ln)
            if m and m.group(1) in r:
                r[m.group(1)] = int(m.group(2))
        out[k] = [r[n] for n in _RES] + [0, sum(not ln.lstrip().startswith(".") for ln in lines)]
    name = None  # the occupancy stands in the comment block after the kernel's code
    for line in open(path, errors="replace"):
        m = re.match(r"^([A-Za-z_][\w$.]*):", line)
        if m and m.group(1) in out:
            name = m.group(1)
        m = re.match(r"^; Occupancy: (\d+)", line)
        if m and name:
            out[name][4] = int(m.group(1))
    return out


def demangle(syms):
    # (c++filt does not know DF16b, the bf16 type: Dh, half, stands in for it)
    r = subprocess.run(["c++filt"], input="\n".join(s.replace("DF16b", "Dh") for s in syms),
                       text=True, capture_output=True).stdout.splitlines()
    return [re.sub(r"\(.*", "", n).replace("void msha::", "").replace("half", "bf16") for n in r]


def table(old, new, a, b):
    ra, rb = resources(old, a), resources(new, b)
    syms = [k for k in sorted(set(a) & set(b)) if a[k] != b[k]]
    print("| kernel | VGPRs | SGPRs | scratch | LDS | occupancy | instructions |")
    print("|---|---|---|---|---|---|---|")
    for k, name in zip(syms, demangle(syms)):
        print(f"| `{name}` | " + " | ".join(f"{x} / {y}" for x, y in zip(ra[k], rb[k])) + " |")


def main(old, new, as_table=False):
    a, b = kernels(old), kernels(new)
    if as_table:
        table(old, new, a, b)
    bad = 0
    for k in sorted(set(a) | set(b)):
        if k not in a or k not in b:
            print(f"only in {'new' if k in b else 'old'}: {k}")
            bad += 1
        elif a[k] != b[k]:
            if not as_table:
                print(f"differs: {k} ({len(a[k])} vs {len(b[k])} lines)")
            bad += 1
    print(f"{len(a)} / {len(b)} symbols, {bad} differences")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:3], as_table="--table" in sys.argv[3:]))
