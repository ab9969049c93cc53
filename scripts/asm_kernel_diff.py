"""Compare the device code of two ``hipcc --cuda-device-only -S`` outputs kernel by kernel.

    python scripts/asm_kernel_diff.py OLD.s NEW.s

Per kernel symbol: the instruction stream (labels, comments, debug and line directives
dropped) and the ``.amdhsa_*`` resource block (VGPRs, SGPRs, LDS, scratch).  Symbol order
and line metadata may differ; anything else is reported.  Exit status 1 on a difference.
"""
from __future__ import annotations

import re
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


def main(old, new):
    a, b = kernels(old), kernels(new)
    bad = 0
    for k in sorted(set(a) | set(b)):
        if k not in a or k not in b:
            print(f"only in {'new' if k in b else 'old'}: {k}")
            bad += 1
        elif a[k] != b[k]:
            print(f"differs: {k} ({len(a[k])} vs {len(b[k])} lines)")
            bad += 1
    print(f"{len(a)} / {len(b)} symbols, {bad} differences")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:3]))
