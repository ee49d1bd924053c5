#!/usr/bin/env python3
"""Per-kernel comparison of two builds' device assembly of one translation unit (a refactor's check: same code, or how far apart).
    hipcc <the Makefile's CXXFLAGS> -DRXHIP_TU_D=4 --cuda-device-only -S -o old_d4.s <old tree>/rxinfer.jl_amd/csrc/tu_lgssm.hip   (and new_d4.s)
    python scripts/isa_compare.py old_d4.s new_d4.s [more pairs …] [--all]
Instruction streams are compared with block labels renumbered in order of appearance; identical kernels are counted, the others listed with
instructions old / new, VGPRs, SGPRs, LDS and scratch (`--all` lists the identical ones too)."""
import re
import shutil
import subprocess
import sys


def kernels(path):
    """{symbol: (instructions, resources)} of every .amdhsa_kernel of an assembly file"""
    body, res, cur, meta = {}, {}, None, None
    for line in open(path):
        s = line.split(";")[0].strip()
        if not s:
            continue
        m = re.match(r"\.amdhsa_kernel\s+(\S+)", s)
        if m:
            meta = m.group(1)
            res[meta] = {}
            continue
        if meta:
            if s == ".end_amdhsa_kernel":
                meta = None
            else:
                m = re.match(r"\.amdhsa_(next_free_vgpr|next_free_sgpr|group_segment_fixed_size|private_segment_fixed_size)\s+(\S+)", s)
                if m:
                    res[meta][m.group(1)] = m.group(2)
            continue
        m = re.match(r"([A-Za-z_][\w$.]*):$", s)
        if m and not s.startswith(".L"):
            cur = m.group(1)
            body[cur] = []
            continue
        if cur is None or s.startswith(".") and not s.startswith(".LBB"):
            continue
        body[cur].append(s)
        if s == "s_endpgm":
            cur = None
    return {k: (normalise(body[k]), res[k]) for k in res if k in body}


def normalise(lines):
    names = {}
    ren = lambda m: names.setdefault(m.group(0), f".L{len(names)}")
    return [re.sub(r"\.LBB\d+_\d+", ren, s) for s in lines]


def demangle(sym):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    name = subprocess.check_output([tool, sym], text=True).strip() if tool else sym
    return name.replace("void rxhip::", "").split("(")[0][:110]


def count(lines):
    return sum(1 for s in lines if not s.endswith(":"))


def main():
    files = [a for a in sys.argv[1:] if not a.startswith("--")]
    show_all = "--all" in sys.argv
    print(f"{'kernel':110s} {'instr old/new':>15s} {'VGPR':>9s} {'SGPR':>9s} {'LDS':>13s} {'scratch':>9s}  tier")
    for old, new in zip(files[0::2], files[1::2]):
        a, b = kernels(old), kernels(new)
        same = 0
        print(f"== {old} against {new}: {len(a)} / {len(b)} kernels")
        for k in sorted(set(a) | set(b)):
            name = demangle(k)
            if k not in a or k not in b:
                print(f"{name:110s} only in {'old' if k in a else 'new'}")
                continue
            (ia, ra), (ib, rb) = a[k], b[k]
            ident = ia == ib
            same += ident
            if ident and not show_all:
                continue
            pair = lambda f: f"{ra.get(f, '?')}/{rb.get(f, '?')}"
            print(f"{name:110s} {count(ia):7d}/{count(ib):<7d} {pair('next_free_vgpr'):>9s} {pair('next_free_sgpr'):>9s} "
                  f"{pair('group_segment_fixed_size'):>13s} {pair('private_segment_fixed_size'):>9s}  {'A' if ident else 'B'}")
        print(f"   identical instruction streams: {same} of {len(set(a) | set(b))}")


if __name__ == "__main__":
    main()
