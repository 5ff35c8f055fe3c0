"""tools/asm_diff.py PARENT_TREE [--variants] [FILE.hip ...] -- device code of this tree against another checkout, file by file.

Compiles every source of so-net_amd/csrc/Makefile's SRCS (or the files named) in both trees with the Makefile's FLAGS plus
--cuda-device-only -S, drops the lines that hold the per-translation-unit id (__hip_cuid_), and prints one line per file: identical,
or the number of differing lines and the kernels they fall in.  For a refactor that must leave the kernels alone; PARENT_TREE is a
checkout of the commit to compare with (git worktree add DIR COMMIT).  Exit status 1 if any file differs."""
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


def main():
    args = [a for a in sys.argv[1:] if a != '--variants']
    extra = ['-DSONET_VARIANTS'] if '--variants' in sys.argv else []
    parent, srcs = os.path.abspath(args[0]), args[1:] or make_var(ROOT, 'SRCS')
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(os.cpu_count() or 4) as pool:
        res = list(pool.map(lambda s: compare(parent, s, extra, tmp), srcs))
    print('\n'.join(res))
    return 1 if any('identical' not in r for r in res) else 0


if __name__ == '__main__':
    sys.exit(main())
