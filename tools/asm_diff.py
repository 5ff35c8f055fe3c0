"""tools/asm_diff.py PARENT_TREE [--variants] [--by-kernel] [FILE.hip ...] -- device code of this tree against another checkout, file by file
or, with --by-kernel, function by function over all sources (for a change that moves kernels between files or renames them).

Compiles every source of so-net_amd/csrc/Makefile's SRCS (or the files named) in both trees with the Makefile's FLAGS plus
--cuda-device-only -S, drops the lines that hold the per-translation-unit id (__hip_cuid_), and prints one line per file: identical,
or the number of differing lines and the kernels they fall in.  For a refactor that must leave the kernels alone; PARENT_TREE is a
checkout of the commit to compare with (git worktree add DIR COMMIT).  Exit status 1 if any file differs.

--by-kernel: the text of every function symbol (from its "Begin function" line to the next one: code, kernel descriptor, register / LDS /
scratch / occupancy summary) over ALL SRCS of either tree, whichever file it sits in.  What is numbered per translation unit is
normalised (.LBB<n>_<m> to the order of the labels in the function, .Lfunc_end<n>, .Ltmp<n>, the names of static LDS symbols, the .section lines, the function's own name) and every
function of the parent is compared with the one of this tree that tests/golden/launch/renamed.txt (old mangled name -> new, one pair per
line) names for it, else with the one of the same name.  Prints per
source file of this tree how many of its functions are identical and names every one that differs (with the number of differing lines
and, for both sides, VGPRs, AGPRs, SGPRs, static LDS bytes, scratch bytes and occupancy from the function's summary comments),
is new, or is gone.  Exit status 1 if any function differs or exists on one side only."""
import difflib
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make_var(tree, name):
    txt = open(os.path.join(tree, 'so-net_amd', 'csrc', 'Makefile')).read().replace('\\\n', ' ')
    return re.search(r'^%s\s*:=\s*(.*)$' % name, txt, re.M).group(1).replace('$(ARCH)', 'gfx950').split()


def asm(tree, src, extra, out):
    subprocess.check_call(['/opt/rocm/bin/hipcc'] + make_var(tree, 'FLAGS') + extra + ['--cuda-device-only', '-S', src, '-o', out],
                          cwd=os.path.join(tree, 'so-net_amd', 'csrc'))
    return [l for l in open(out).read().split('\n') if '__hip_cuid_' not in l]


def compare(parent, src, extra, tmp):
    old = asm(parent, src, extra, os.path.join(tmp, 'old_' + src + '.s'))
    new = asm(ROOT, src, extra, os.path.join(tmp, 'new_' + src + '.s'))
    if old == new:
        return '%-24s identical (%d lines)' % (src, len(new))
    for side, lines in (('old', old), ('new', new)):
        open(os.path.join(tmp, side + '_' + src + '.txt'), 'w').write('\n'.join(lines))
    d = subprocess.run(['diff', '--old-line-format=o%dn\n', '--new-line-format=n%dn\n', '--unchanged-line-format=',
                        os.path.join(tmp, 'old_' + src + '.txt'), os.path.join(tmp, 'new_' + src + '.txt')],
                       stdout=subprocess.PIPE, universal_newlines=True).stdout.split()
    kernels = set()
    for side, lines in (('o', old), ('n', new)):
        where, cur = [], '(file scope)'
        for l in lines:                                   # a line belongs to the last function label above it
            m = re.match(r'([A-Za-z_]\w*):', l)
            cur = m.group(1) if m else cur
            where.append(cur)
        kernels |= {where[int(x[1:]) - 1] for x in d if x[0] == side}
    return '%-24s %d differing lines of %d in: %s' % (src, len(d), len(new), ', '.join(sorted(kernels)))


def renamed():
    """{old symbol: [new symbols]} of tests/golden/launch/renamed.txt"""
    path = os.path.join(ROOT, 'tests', 'golden', 'launch', 'renamed.txt')
    out = {}
    for l in (open(path).read().split('\n') if os.path.exists(path) else []):
        if l.strip():
            out.setdefault(l.split()[0], []).append(l.split()[1])      # (a kernel split in two is listed once per successor)
    return out


def functions(lines, src):
    """{symbol: [(src, normalised lines)]} of one assembly file; the function's own name reads @self"""
    out, cur, sym = {}, None, None
    for l in lines:
        m = re.search(r'; -- Begin function (\S+)', l)
        if m:
            sym = m.group(1)
            cur = out.setdefault(sym, [])
            cur.append((src, []))
        if re.match(r'\s*\.(section\s+\.AMDGPU\.gpr_maximums|amdgpu_metadata|section\s+\.bss)', l):
            cur = None                                          # (end of the last function: file-level tables follow)
        if cur is None or re.match(r'\s*\.section\s+\.text', l):
            continue
        l = l.replace(sym, '@self')
        l = re.sub(r'\.(LBB|Lfunc_end|Lfunc_begin|Ltmp)\d+', r'.\1', l)
        l = re.sub(r'\s+', ' ', re.sub(r'\bBB\d+_', 'BB_', l))                               # (comments: "Header=BB12_3", padded to a column)
        l = re.sub(r'\b(_ZZ\w+|llvm\.amdgcn\.[\w.]+\.lds\b)', 'LDS', l)                 # static LDS symbols carry the enclosing function's name
        cur[-1][1].append(l)
    for blocks in out.values():                              # block numbers: an empty fall-through block more or less shifts them all
        for _, body in blocks:
            order = {}
            for l in body:
                m = re.match(r'\.LBB_(\d+):', l)
                if m:
                    order.setdefault(m.group(1), str(len(order)))
            for i, l in enumerate(body):
                code, sep, comment = l.partition(';')
                code = re.sub(r'\.LBB_(\d+)', lambda m: '.LBB_' + order.get(m.group(1), '?' + m.group(1)), code)
                body[i] = code + sep + re.sub(r'(%bb\.|BB_)\d+', r'\1', comment)
            body[:] = [l for l in body if not l.startswith('; %bb.')]          # (the comment in front of a fall-through block)
    return out


def resources(blocks):
    """'VGPR a (+ AGPR), SGPR, LDS, scratch, occupancy' of a function, from the summary comments behind its code"""
    text = '\n'.join(l for b in blocks for l in b)
    get = lambda key: '/'.join(re.findall(r'; %s: (\d+)' % key, text)) or '?'
    return 'VGPR %s AGPR %s SGPR %s LDS %s scratch %s occupancy %s' % tuple(
        get(k) for k in ('NumVgprs', 'NumAgprs', 'TotalNumSgprs', 'LDSByteSize', 'ScratchSize', 'Occupancy'))


def by_kernel(parent, extra, tmp, pool):
    names = renamed()
    sides = []
    for tag, tree in (('old', parent), ('new', ROOT)):
        srcs = make_var(tree, 'SRCS')
        texts = list(pool.map(lambda s: asm(tree, s, extra, os.path.join(tmp, '%s_%s.s' % (tag, s))), srcs))
        fns = {}
        for s, t in zip(srcs, texts):
            for sym, blocks in functions(t, s).items():
                fns.setdefault(sym, []).extend(blocks)
        sides.append(fns)
    old, new = sides
    res, bad, seen = {}, 0, set()                             # per source file of this tree: [identical, [message]]
    for sym, to in sorted((sym, to) for sym in old for to in names.get(sym, [sym])):     # every function of the parent against what replaces it
        seen.add(to)
        o, n = sorted(b[1] for b in old[sym]), sorted(b[1] for b in new.get(to, []))
        r = res.setdefault(new[to][0][0] if n else old[sym][0][0] + ' (parent)', [0, []])
        was = ('%s in %s' % (sym, old[sym][0][0])) if to != sym else old[sym][0][0]
        if o == n:
            r[0] += len(n)
        elif not n:
            r[1].append('%s: only in the parent' % sym)
        else:
            nd = sum(1 for a, b in zip(o, n) for d in difflib.ndiff(a, b) if d[0] in '+-')
            r[1].append('%s: %d differing lines of %d (was %s)\n        parent: %s\n        here:   %s' % (to, nd, sum(map(len, n)), was, resources(o), resources(n)))
    for sym in sorted(set(new) - seen):
        res.setdefault(new[sym][0][0], [0, []])[1].append('%s: only in this tree' % sym)
    for where in sorted(res):
        same, msgs = res[where]
        print('%-24s %d functions identical%s' % (where, same, '' if not msgs else ', %d not:' % len(msgs)))
        for m in msgs:
            print('    ' + m)
        bad += len(msgs)
    print('%d functions of this tree, %d of the parent; %d differ or exist on one side only' % (sum(map(len, new.values())), sum(map(len, old.values())), bad))
    return 1 if bad else 0


def main():
    args = [a for a in sys.argv[1:] if a not in ('--variants', '--by-kernel')]
    extra = ['-DSONET_VARIANTS'] if '--variants' in sys.argv else []
    if '--by-kernel' in sys.argv:
        with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(min(16, os.cpu_count() or 4)) as pool:
            return by_kernel(os.path.abspath(args[0]), extra, tmp, pool)
    parent, srcs = os.path.abspath(args[0]), args[1:] or make_var(ROOT, 'SRCS')
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(os.cpu_count() or 4) as pool:
        res = list(pool.map(lambda s: compare(parent, s, extra, tmp), srcs))
    print('\n'.join(res))
    return 1 if any('identical' not in r for r in res) else 0


if __name__ == '__main__':
    sys.exit(main())
