#!/usr/bin/env python3
"""The memory operations, the s_waitcnt that name vmcnt, the barriers (with the wait in front of each) and the block labels of one loop of a
kernel, old build against new, from the device assembly scripts/isa_compare.py reads.
    python scripts/isa_waits.py old_d4.s new_d4.s "k_backward_sh_rev<4, 4, 4, 2>" last      (the last loop of the kernel)
    python scripts/isa_waits.py old_d4.s new_d4.s "k_forward0_ck<4, 4, true, 1>" fp64       (the loop with the most fp64 arithmetic)
Numbers are line offsets from the loop header.  The closing lines count the operations and say whether the two listings agree once register
numbers and offsets are taken out."""
import re
import sys

import isa_compare as ic

FP64 = re.compile(r"v_(fma|fmac|mul|add)_f64")
MEM = re.compile(r"(global|buffer|flat|scratch)_(load|store|atomic)")


def loop_of(lines, which):
    """[header, back edge] of the chosen loop: the widest loop that ends at the kernel's last back edge, or the loop with the most fp64 operations"""
    at = {s[:-1]: i for i, s in enumerate(lines) if s.endswith(":")}
    loops = []
    for i, s in enumerate(lines):
        m = re.match(r"s_cbranch_\w+\s+(\S+)", s) or re.match(r"s_branch\s+(\S+)", s)
        if m and at.get(m.group(1), i) < i:
            loops.append((at[m.group(1)], i))
    if which == "last":
        end = max(e for _, e in loops)
        return min(b for b, e in loops if e == end), end
    return max(loops, key=lambda be: sum(1 for s in lines[be[0]:be[1]] if FP64.match(s)))


def listing(lines):
    out = []
    for i, s in enumerate(lines):
        if s.endswith(":") or s.startswith("s_cbranch") or MEM.match(s) or (s.startswith("s_waitcnt") and "vmcnt" in s):
            out.append((i, s))
        elif s.startswith("s_barrier"):
            out.append((i, f"s_barrier   <- {lines[i - 1]}"))
    return out


def shape(rows):
    """the listing without register numbers, offsets and label names"""
    return [re.sub(r"\.L\d+", ".L", re.sub(r"\s.*", "", s) if MEM.match(s) else s) for _, s in rows if not s.endswith(":") and not s.startswith("s_cbranch")]


def main():
    old, new, pat, which = sys.argv[1:5]
    shapes = []
    for tag, path in (("old", old), ("new", new)):
        ks = ic.kernels(path)
        sym = next(k for k in ks if ic.demangle(k).startswith(pat))
        lines = ks[sym][0]
        b, e = loop_of(lines, which)
        body = lines[b:e + 1]
        rows = listing(body)
        print(f"== {tag} {ic.demangle(sym)}: loop of {len(body)} lines ({sum(1 for s in body if FP64.match(s))} fp64 operations) ==")
        for i, s in rows:
            print(f"{i:5d}  {s}")
        ops = [s for _, s in rows]
        bar = [s for s in ops if s.startswith("s_barrier")]
        print(f"   loads {sum('_load' in s for s in ops)}, stores {sum('_store' in s for s in ops)}, waits that name vmcnt {sum(s.startswith('s_waitcnt') for s in ops)}, "
              f"of them vmcnt(0) {sum(s.startswith('s_waitcnt') and 'vmcnt(0)' in s for s in ops)}, barriers {len(bar)}, "
              f"barriers behind a wait other than `s_waitcnt lgkmcnt(0)` {sum(not s.endswith('<- s_waitcnt lgkmcnt(0)') for s in bar)}")
        shapes.append(shape(rows))
    print(f"== memory operations, vmcnt waits and barriers in the same order in both: {shapes[0] == shapes[1]} ==")


if __name__ == "__main__":
    main()
