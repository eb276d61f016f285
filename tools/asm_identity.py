#!/usr/bin/env python3
"""Do two builds hold the same kernel code?  Compares the gfx950 assembly that `hipcc -save-temps` (or `--cuda-device-only -S`) leaves
function by function -- body and `.amdhsa_*` descriptor block -- after dropping comments, the numbers of local labels and the
function's own name, whatever the order of the functions and whichever file of a side holds them.  A refactor that only moves code
must come out with 0 different.

    hipcc <CXXFLAGS of csrc/Makefile> -save-temps -c ai_ncut.hip      (in each tree, in a scratch directory)
    python tools/asm_identity.py [--rename OLD=NEW ...] OLD.s[,OLD2.s...] NEW.s[,NEW2.s...]

Lines: DIFF (exit status 1), SWAP (same length, same mnemonics, the only differing lines have the two source operands of a commutative
instruction exchanged: the same bits; counted per mnemonic, exit status 0), under a DIFF one line with the descriptor lines and the instruction counts per mnemonic that differ, ONLY-OLD / ONLY-NEW for a kernel of the project's
anonymous namespace that one side lacks.  `--rename OLD=NEW` (names as these lines print them) compares a kernel that the old side
calls OLD with the one the new side calls NEW."""
import re, sys, subprocess

COMMUTATIVE = re.compile(r'^[vs]_(add|mul|and|or|xor|xnor|min|max)(_|$)')

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
        l = l.replace(name, '<self>')  # a renamed kernel differs in nothing but this
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
    s = re.sub(r'\(anonymous namespace\)::', '', subprocess.run(['c++filt', n], capture_output=True, text=True).stdout.strip()).split('(')[0]
    return s[5:] if s.startswith('void ') else s  # an instance of a template is printed with its return type

def swaps(vo, vn):
    """None unless the bodies differ only by exchanged source operands of commutative instructions; else {mnemonic: lines}."""
    if len(vo) != len(vn):
        return None
    count = {}
    for a, b in zip(vo, vn):
        if a == b:
            continue
        (ma, _, ra), (mb, _, rb) = a.partition(' '), b.partition(' ')
        oa, ob = ra.split(', '), rb.split(', ')
        if ma != mb or not COMMUTATIVE.match(ma) or len(oa) < 3 or oa[:-2] != ob[:-2] or oa[-2:] != ob[:-3:-1]:
            return None
        count[ma] = count.get(ma, 0) + 1
    return count

def resources(vo, vn):
    """What a DIFF kernel kept: the `.amdhsa_*` descriptor lines (registers, LDS, scratch, accum_offset) and the per-mnemonic
    instruction counts that differ, old -> new; vector and memory mnemonics (v_*, ds_*, global/flat/buffer/scratch_*, s_load*) first."""
    def split(v):
        desc = {l.split(' ')[0]: l.partition(' ')[2] for l in v if l.startswith('.amdhsa_')}
        count = {}
        for l in v:
            if not l.startswith('.') and not l.endswith(':'):
                count[l.split(' ')[0]] = count.get(l.split(' ')[0], 0) + 1
        return desc, count
    (do, co), (dn, cn) = split(vo), split(vn)
    heavy = lambda m: bool(re.match(r'(v_|ds_|global_|flat_|buffer_|scratch_|s_load|s_buffer_load)', m))
    show = lambda o, n, keys: ' '.join('%s:%s->%s' % (k, o.get(k, 0), n.get(k, 0)) for k in keys) or 'equal'
    moved = sorted(k for k in set(co) | set(cn) if co.get(k, 0) != cn.get(k, 0))
    return 'descriptor %s | vector+memory %s | other %s' % (show(do, dn, sorted(k for k in set(do) | set(dn) if do.get(k) != dn.get(k))),
                                                            show(co, cn, [k for k in moved if heavy(k)]), show(co, cn, [k for k in moved if not heavy(k)]))

args, renames = sys.argv[1:], {}
while args and args[0] == '--rename':
    o, _, n = args[1].partition('=')
    renames[o] = n
    args = args[2:]
old, new = load(args[0]), load(args[1])
ours = lambda n: n.startswith('_ZN12_GLOBAL__N_1')
by_name = {}
for n in new:
    by_name.setdefault(dem(n), []).append(n)
pairs, only_old, matched = [], [], set()
for n in sorted(set(old) | set(new)):
    if n in old and n in new:
        pairs.append((n, n))
    elif n in old and ours(n):
        targets = by_name.get(renames.get(dem(n)), [])
        if len(targets) == 1:
            pairs.append((n, targets[0]))
            matched.add(targets[0])
        else:
            only_old.append(n)
for n in only_old:
    print('ONLY-OLD ' + dem(n))
for n in sorted(new):
    if n not in old and ours(n) and n not in matched:
        print('ONLY-NEW ' + dem(n))
same = diff = swapped = 0
for no, nn in pairs:
    label = dem(no) if no == nn else '%s -> %s' % (dem(no), dem(nn))
    for po, vo in old[no]:
        for pn, vn in new[nn]:
            sw = None if vo == vn else swaps(vo, vn)
            if vo == vn:
                same += 1
                if no != nn:
                    print('RENAMED', label, po.split('/')[-1], pn.split('/')[-1], 'identical')
            elif sw is not None:
                swapped += 1
                print('SWAP', label, po.split('/')[-1], pn.split('/')[-1], len(vo), ' '.join('%s:%d' % kv for kv in sorted(sw.items())))
            else:
                diff += 1
                print('DIFF', label, po.split('/')[-1], pn.split('/')[-1], len(vo), len(vn))
                print('    ' + resources(vo, vn))
nk = sum(1 for no, nn in pairs if ours(nn))
print('compared %d function pairs (%d project kernels by name): %d identical, %d operand swaps only, %d different'
      % (same + swapped + diff, nk, same, swapped, diff))
sys.exit(1 if diff else 0)
