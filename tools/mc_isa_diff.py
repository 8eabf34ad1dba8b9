#!/usr/bin/env python3
"""Compare the gfx950 kernels of two sets of assembly files (hipcc --cuda-device-only -S), kernel by kernel:
    python3 tools/mc_isa_diff.py parent.s -- branch_a.s branch_b.s
For every kernel symbol: the instruction stream (comments, .file / .loc / .cfi lines dropped, the function number of .LBB<n>_ labels
replaced) and the .amdhsa_* block must be the same.  Prints one row per kernel
(instructions, VGPRs, SGPRs, scratch, LDS) and exits non-zero on any difference or on differing symbol sets."""
import re
import sys


def kernels(paths):
    body, desc = {}, {}
    for path in paths:
        lines = open(path).read().split("\n")
        for i, line in enumerate(lines):
            m = re.match(r"^(_Z\w+):\s*(;.*)?$", line)
            if m and any(f".type\t{m.group(1)},@function" in l for l in lines[max(0, i - 6):i]):
                out = []                                            # the code ends where the descriptor's section begins
                for l in lines[i + 1:]:
                    s = l.strip()
                    if s.startswith(".section") or s.startswith(".Lfunc_end"):
                        break
                    if s and not s.startswith(";") and not re.match(r"\.(file|loc|cfi_)", s):
                        out.append(re.sub(r"\.L(BB|tmp)\d+", r".L\1N", re.sub(r"\s+;.*$", "", s)))
                body[m.group(1)] = out
            m = re.match(r"^\s*\.amdhsa_kernel (\w+)", line)
            if m:
                end = next(k for k in range(i, len(lines)) if lines[k].strip().startswith(".end_amdhsa_kernel"))
                desc[m.group(1)] = [l.strip() for l in lines[i + 1:end]]
    return {k: (body[k], desc[k]) for k in desc}


def field(desc, key):
    for l in desc:
        if l.startswith(key + " "):
            return l.split()[-1]
    return "-"


def main():
    cut = sys.argv.index("--")
    old, new = kernels(sys.argv[1:cut]), kernels(sys.argv[cut + 1:])
    bad = sorted(set(old) ^ set(new))
    for k in bad:
        print("only in", "parent" if k in old else "branch", k)
    print("| kernel | instructions | next-free VGPR | next-free SGPR | scratch | LDS | same |")
    print("|---|---|---|---|---|---|---|")
    for k in sorted(set(old) & set(new)):
        same = old[k] == new[k]
        if not same:
            bad.append(k)
        d = new[k][1]
        n_insn = sum(1 for l in new[k][0] if not l.endswith(":") and not l.startswith("."))
        print(f"| {k} | {n_insn} | {field(d, '.amdhsa_next_free_vgpr')} | {field(d, '.amdhsa_next_free_sgpr')} | "
              f"{field(d, '.amdhsa_private_segment_fixed_size')} | {field(d, '.amdhsa_group_segment_fixed_size')} | {'yes' if same else 'NO'} |")
    print(f"{len(old)} kernels in the parent, {len(new)} in the branch, {len(bad)} differ")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
