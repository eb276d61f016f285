#!/usr/bin/env python3
"""Do two builds hold the same kernel code?  Compares the gfx950 assembly that `hipcc -save-temps` leaves (*-hip-amdgcn-*.s) function
by function -- body and `.amdhsa_*` descriptor block -- after dropping comments and the numbers of local labels, whatever the order
of the functions and whichever file of a side holds them.  A refactor that only moves code must come out with 0 different.

    hipcc <CXXFLAGS of csrc/Makefile> -save-temps -c ai_ncut.hip      (in each tree, in a scratch directory)
    python tools/asm_identity.py OLD.s[,OLD2.s...] NEW.s[,NEW2.s...]  -> DIFF / ONLY-OLD / ONLY-NEW lines, exit status 1 on a DIFF"""
import re, sys, subprocess

def funcs(path):
    out, name, buf = {}, None, []
    for line in open(path):
        m = re.match(r'\t\.globl\t(\S+)\s*; -- Begin function', line)
        if m:
            name, buf = m.group(1), []
            continue
        if name is None:
            continue
        if '; -- End function' in line:
            out[name] = buf
            name = None
            continue
        line = line.split(';')[0]  # comments carry IR block names
        l = re.sub(r'BB\d+_(\d+)', r'BB#_\1', line)
        l = re.sub(r'\.Lfunc_(begin|end)\d+', r'.Lfunc_\1#', l)
        l = re.sub(r'\.Ltmp\d+', '.Ltmp#', l)
        l = re.sub(r'\s+', ' ', l).strip()
        if l:
            buf.append(l)
    return out

def load(spec):
    d = {}
    for p in spec.split(','):
        for k, v in funcs(p).items():
            d.setdefault(k, []).append((p, v))
    return d

def dem(n):
    return re.sub(r'\(anonymous namespace\)::', '', subprocess.run(['c++filt', n], capture_output=True, text=True).stdout.strip()).split('(')[0]

old, new = load(sys.argv[1]), load(sys.argv[2])
ours = lambda n: re.search(r'GLOBAL__N_1\d+f?k_', n) is not None
same = diff = 0
for n in sorted(set(old) | set(new)):
    if n not in old or n not in new:
        if ours(n):
            print(('ONLY-OLD ' if n in old else 'ONLY-NEW ') + dem(n))
        continue
    for po, vo in old[n]:
        for pn, vn in new[n]:
            if vo == vn:
                same += 1
            else:
                diff += 1
                print('DIFF', dem(n), po.split('/')[-1], pn.split('/')[-1], len(vo), len(vn))
nk = sum(1 for n in new if ours(n) and n in old)
print('compared %d function pairs (%d project kernels by name): %d identical, %d different' % (same + diff, nk, same, diff))
sys.exit(1 if diff else 0)
