#!/usr/bin/env python3
"""Compare two device assembly listings function by function:  compare_kernel_asm.py OLD.s NEW.s

The listings are hipcc's device-only -S output, made with the build's flags (superodom_amd/build.py COMMON), e.g.
    hipcc --offload-arch=gfx950 -x hip --cuda-device-only -S -O3 -std=c++17 -fPIC -ffp-contract=off \\
          superodom_amd/csrc/feature_kernels.hip -o feature_kernels.s
A function is what lies between its `.type NAME,@function` and its `.Lfunc_end` label, plus its `.amdhsa_kernel` descriptor
(registers, LDS, scratch).  Comments, debug directives and the function's number in local labels (.LBB<n>_<m>: it counts the
functions in front) are dropped before the comparison.  Prints one line per function and a summary; exit status 1 when a
function differs or is in one listing only."""
import re
import subprocess
import sys

DEBUG = (".loc", ".file", ".cfi_")


def functions(path):
    """{name: normalised lines} in the listing's order; a line that is neither a label nor a directive is an instruction"""
    out, cur = {}, None
    for line in open(path):
        line = re.sub(r"\.LBB\d+_", ".LBB_", line.split(";")[0].split("//")[0]).strip()
        m = re.match(r"\.type\s+(\S+),@function", line) or re.match(r"\.amdhsa_kernel\s+(\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif line.startswith((".Lfunc_end", ".end_amdhsa_kernel")):
            cur = None
        elif cur is not None and line and not line.startswith(DEBUG):
            cur.append(line)
    return out


def main(old_path, new_path):
    old, new = functions(old_path), functions(new_path)
    names = list(old) + [n for n in new if n not in old]
    try:
        pretty = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    except (OSError, subprocess.CalledProcessError):
        pretty = names
    count = lambda f: sum(1 for l in f if not l.startswith(".") and not l.endswith(":"))
    bad = 0
    for name, shown in zip(names, pretty):
        a, b = old.get(name), new.get(name)
        verdict = "identical" if a == b else "changed" if a is not None and b is not None else "missing in " + ("OLD" if a is None else "NEW")
        bad += verdict != "identical"
        print(f"{verdict:10s} {'-' if a is None else count(a):>6} {'-' if b is None else count(b):>6}  {shown}")
    print(f"{new_path}: {len(names)} functions, {len(names) - bad} identical, {bad} changed or missing")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
