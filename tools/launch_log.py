"""tools/launch_log.py TREE [--variants] [--bn] [--upconv] [--full] [--summary] [--sanitize] -- what the layer launchers of a checkout launch, without a GPU.

Compiles every source of TREE's so-net_amd/csrc/Makefile SRCS host-only (the Makefile's FLAGS plus --cuda-host-only), links them with a
recording stand-in for the HIP runtime (tools/launch_stub.cpp) and a driver with its own main (tools/launch_driver.cpp: the C ABI of
the pointmlp / pointresnet / wgrad launchers over the networks' channel pairs, B x L sizes, optional features and refused combinations),
runs it and prints every case: arguments, return code, sonet_last_error() when refused, and each launch as
kernel:grid[:block[:LDS bytes]] (kernel = index into the K table at the top; ",1" grid / block tails and a block of 256 without LDS
dropped; m = a hipMemsetAsync; E = index into the table of error texts; consecutive cases with one outcome share a line).

  == base                      every case, CU count 256, no knob
  == LAUNCH_LOG_CUS=...        the cases that differ from base with another CU count / a failing CU query
  == bn passes: ...            with --bn (without it the output is what it was before this half existed, byte for byte): the same for the family of the BatchNorm / ReLU passes (the driver's "@bn" half: the element-wise passes, the
                               coefficient kernels, the eval-mode head kernels, the pooled sparse gradient), behind K / E tables of its own
  == upconv: ...               with --upconv (appended the same way): the decoder's up-convolutions (the driver's "@upconv" half: the two
                               pack sizes and pack kernels, the forward, the input gradient, the weight gradient and its workspace size;
                               a size function's return value stands where a return code does)
  --variants: the -DSONET_VARIANTS build.  base lists the cases that differ from the product build's; then one section per SONET_*
              knob setting (each value the code distinguishes and one it rejects) over the launchers that read it: per group of cases
              (entry point, features, channel pair) the number of cases that differ from base and a digest of the group's text --
              --full prints the cases themselves.
  --summary:  the outline only (summarise() below): per section and entry point the number of lines and a digest of them.
  --sanitize: the driver and the host code are built with -fsanitize=address,undefined (a stand-alone program, nothing preloaded).

tests/test_launch_log_cpu.py holds the output for the working tree against tests/golden/launch/, recorded from the parent of the
host-side refactor (git worktree add DIR COMMIT; tools/launch_log.py DIR): NAME.txt.xz is the whole output (27,000 lines, kept
compressed: lzma.open(path, 'wt', preset=9)), NAME.summary.txt its outline.  A changed dispatch shows as a diff of the outline, and the
failing test prints the differing cases themselves."""
import hashlib
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = '/opt/rocm/bin/hipcc'
CXX = '/opt/rocm/llvm/bin/clang++'
# (-fno-sanitize=function: a kernel launched through a non-type template parameter -- common.hpp's launch_lds_once -- is a call through a
#  pointer to the kernel's handle, which the function sanitizer takes for undefined behaviour: hipcc then drops the launch altogether)
SANITIZE = ['-fsanitize=address,undefined', '-fno-sanitize=function']

CUS = ['304', '64', '4', 'fail']
# knob -> (values, group prefixes of the launchers that read it)
X3 = ['sonet_pointmlp_x3', 'sonet_pointmlp_h3_']
KNOBS = [
    ('SONET_POINTMLP_H3R', ['0', '1', 'x'], X3),
    ('SONET_POINTMLP_NC', ['2', '1', 'x'], X3),
    ('SONET_POINTMLP_YSPLIT', ['1', '2', '3', '4', '0', '7'], X3),
    ('SONET_POINTMLP_MT', ['1', '2', '4', '6', '8', '3'], X3 + ['sonet_pointmlp_f32']),
    ('SONET_POINTMLP_S', ['1', '2', '4', '3'], X3 + ['sonet_pointmlp_f32']),
    ('SONET_POINTMLP_ABLATE', ['1', '2', '3', '4', '7', '5'], ['sonet_pointmlp_f32']),
    ('SONET_POINTMLP_KERNEL', ['wlds', 'lean'], ['sonet_pointmlp_f32']),
    ('SONET_BF16_MT', ['1', '2', '4', '6', '12', '5'], ['sonet_pointmlp_bf16']),
    ('SONET_BF16_ABL', ['1'], ['sonet_pointmlp_bf16']),
    ('SONET_BF16_S', ['1', '2', '3'], ['sonet_pointmlp_bf16']),
    ('SONET_BF16_YSPLIT', ['1', '2', '3', '4', '0'], ['sonet_pointmlp_bf16']),
    ('SONET_BF16_XREG', ['1', '2', '0'], ['sonet_pointmlp_bf16']),
    ('SONET_BF16_STREAM', ['0', '1'], ['sonet_pointmlp_bf16']),
    ('SONET_BF16_SYNC', ['0', '1'], ['sonet_pointmlp_bf16']),
    ('SONET_BF16_NXB', ['3', '2'], ['sonet_pointmlp_bf16']),
    ('SONET_BF16_POOL_NS', ['1', '2', '4', '0', '5'], ['sonet_pointmlp_bf16_pool']),
    ('SONET_BF16_POOL_ABL', ['1'], ['sonet_pointmlp_bf16_pool']),
    ('SONET_H3P_SHAPE', ['4,2,2', '4,1,2', '2,1,2', '8,2,1', '6,2,1', '12,1,1', '3,1,1', 'x'], ['sonet_pointmlp_h3p']),
    ('SONET_H3P_NSLAB', ['1', '2', '4', '8', '0'], ['sonet_pointmlp_h3p']),
    ('SONET_H3P_ABL', ['1'], ['sonet_pointmlp_h3p']),
    ('SONET_H3P_PROF', ['0x1000'], ['sonet_pointmlp_h3p']),
    ('SONET_BF16_FUSED_ABLATE', ['1'], ['sonet_pointresnet_bf16']),
    ('SONET_BF16_POOL2', ['0', '1'], ['sonet_pointresnet_bf16']),
    ('SONET_BF16_POOL2_GRID', ['8', '0'], ['sonet_pointresnet_bf16']),
    ('SONET_FUSED_FREE_CUS', ['8', '-1', '0'], ['sonet_pointresnet_fused']),
    ('SONET_WGRAD_BF16_STREAM', ['0', '1'], ['sonet_wgrad_bf16']),
]
# knobs whose launchers also ask for the CU count: the two together
# the family of the BatchNorm / ReLU passes (the driver's "@bn" half): only the pooled input gradient reads knobs, nothing asks for the CU count
BN_KNOBS = [
    ('SONET_PD_ABL', ['1', '4'], ['sonet_pooled_dgrad']),
    ('SONET_PD_ONE', ['1'], ['sonet_pooled_dgrad']),
    ('SONET_PD_KERNEL', ['4', '5', '3'], ['sonet_pooled_dgrad']),
    ('SONET_PM_CH', ['1', '2', '3'], ['sonet_pooled_dgrad_mfma']),
]
KNOBS_X_CUS = [('SONET_POINTMLP_NC', '2', X3), ('SONET_BF16_XREG', '2', ['sonet_pointmlp_bf16']), ('SONET_BF16_POOL2', '0', ['sonet_pointresnet_bf16']),
               ('SONET_FUSED_FREE_CUS', '8', ['sonet_pointresnet_fused']), ('SONET_FUSED_FREE_CUS', '-1', ['sonet_pointresnet_fused'])]


def make_var(tree, name):
    txt = open(os.path.join(tree, 'so-net_amd', 'csrc', 'Makefile')).read().replace('\\\n', ' ')
    return re.search(r'^%s\s*:=\s*(.*)$' % name, txt, re.M).group(1).replace('$(ARCH)', 'gfx950').split()


def build(tree, variants, sanitize, tmp):
    """the driver linked against TREE's host objects and the stand-in runtime; returns the program's path"""
    tag = ('v' if variants else 'p') + ('s' if sanitize else '')
    extra = (['-DSONET_VARIANTS'] if variants else []) + (SANITIZE + ['-fno-omit-frame-pointer', '-g'] if sanitize else [])
    csrc = os.path.join(tree, 'so-net_amd', 'csrc')
    flags = [f for f in make_var(tree, 'FLAGS') if not f.startswith('--offload-arch')]
    jobs = [([HIPCC] + flags + extra + ['--cuda-host-only', '-c', s, '-o', os.path.join(tmp, '%s_%s.o' % (tag, s))], csrc) for s in make_var(tree, 'SRCS')]
    for s in ('launch_stub.cpp', 'launch_driver.cpp'):
        jobs.append(([CXX, '-std=c++17', '-O1', '-Wall', '-I', tree] + extra + ['-c', os.path.join(ROOT, 'tools', s), '-o', os.path.join(tmp, '%s_%s.o' % (tag, s))], ROOT))
    with ThreadPoolExecutor(min(16, os.cpu_count() or 4)) as pool:
        list(pool.map(lambda j: subprocess.check_call(j[0], cwd=j[1]), jobs))
    exe = os.path.join(tmp, 'launch_driver_' + tag)
    # (--unresolved-symbols: the per-file __hip_fatbin_* symbol of a host-only object; the stand-in never reads it)
    subprocess.check_call([CXX] + [j[0][-1] for j in jobs] + (SANITIZE if sanitize else []) +
                          ['-Wl,--unresolved-symbols=ignore-all', '-o', exe])
    return exe


def recorded_names():
    """{kernel name: the name it is printed under}.  tests/golden/launch/renamed.txt holds "old new" per line for every kernel that was
    renamed or merged after the fixtures were recorded (names only, nothing else goes through it).  A kernel of this tree is printed under
    the FIRST old name the file lists for it, and so is every other old name that became the same kernel: the text of a tree that merged
    two kernels then differs from the recording only where the recording tells the two apart, and `expand` below removes that."""
    path = os.path.join(ROOT, 'tests', 'golden', 'launch', 'renamed.txt')
    pairs = [l.split() for l in open(path).read().split('\n') if l.strip()] if os.path.exists(path) else []
    first = {}
    for old, new in pairs:
        first.setdefault(new, old)
    out = {new: old for new, old in first.items()}
    out.update({old: first[new] for old, new in pairs})
    return out


def expand(text):
    """A recording or an output as one line per case, kernel indices and error indices replaced by what they stand for (kernel names
    through recorded_names()), the K / E tables dropped: what two texts must agree in when kernels were merged or renamed between them
    -- every case, its return code and message, every launch with its kernel, grid, block and LDS size.  Digest lines stay as they are."""
    names = recorded_names()
    K, E, out = {}, {}, []
    for line in text.rstrip('\n').split('\n'):
        m = re.match(r'([KE])(\d+) (.*)$', line)
        if m:
            (K if m.group(1) == 'K' else E)[m.group(2)] = names.get(m.group(3), m.group(3)) if m.group(1) == 'K' else m.group(3)
            continue
        if line.startswith('== ') and 'kernels and refusal texts' in line:
            K, E = {}, {}                                    # (the tables of the second half follow)
            continue
        m = re.match(r'  (.*) (-?\d+)( E\d+)?$', line.split(' | ')[0]) if line.startswith('  ') else None
        if not m:
            out.append(line)
            continue
        items = [K[t.split(':')[0]] + t[len(t.split(':')[0]):] if t != 'm' else t for t in line.split(' | ')[1].split()] if ' | ' in line else []
        tail = m.group(2) + (' ' + E[m.group(3)[2:]] if m.group(3) else '') + (' | ' + ' '.join(items) if items else '')
        out += ['  %s %s' % (c, tail) for c in m.group(1).split(',')]
    return out


def run(exe, env, prefixes=()):
    """{group: [(case, text)]} in the driver's order; text = 'rc [error] | launches' with kernel NAMES"""
    back = recorded_names()                                  # (names are rewritten on OUTPUT: a recording made with renamed.txt in place already
                                                             #  carries the merged names -- record a parent with the file moved aside)
    e = dict((k, v) for k, v in os.environ.items() if not k.startswith('SONET_') and k != 'LAUNCH_LOG_CUS')
    e.update(env)
    out = subprocess.run([exe] + list(prefixes), env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    if out.returncode != 0 or out.stderr.strip():
        raise RuntimeError('driver failed (rc %d) with %r:\n%s' % (out.returncode, env, out.stderr[-4000:]))
    res = {}
    for line in out.stdout.split('\n'):
        if not line:
            continue
        group, case, rc, err, launches = line.split('\t')
        res.setdefault(group, []).append((case, (rc, err, [back.get(t, t) for t in launches.split()])))
    return res


class Names:
    """kernel name -> index in the sorted table of every name seen"""
    def __init__(self, runs):
        seen = set()
        for r in runs:
            for cases in r.values():
                for _, (_, _, toks) in cases:
                    seen |= {t for t in toks if not re.match(r'[\d,]+$', t) and t != 'memset'}
        errors = {err for r in runs for cases in r.values() for _, (_, err, _) in cases if err}
        self.table, self.errors = sorted(seen), sorted(errors)
        self.index = {n: i for i, n in enumerate(self.table)}
        self.eindex = {n: i for i, n in enumerate(self.errors)}

    def text(self, rec):
        rc, err, toks = rec
        items, i = [], 0
        while i < len(toks):
            if toks[i] == 'memset':
                items.append('m')
                i += 1
                continue
            grid, block = (re.sub(r'(,1)+$', '', t) for t in toks[i + 1:i + 3])
            lds = toks[i + 3]
            items.append('%d:%s' % (self.index[toks[i]], grid) + (':' + block if block != '256' or lds != '0' else '') + (':' + lds if lds != '0' else ''))
            i += 4
        return rc + (' E%d' % self.eindex[err] if err else '') + (' | ' + ' '.join(items) if items else '')


def full_section(res, names, base=None):
    """every case (base None) or the cases whose text differs from base's"""
    lines = []
    for group, cases in res.items():
        ref = dict(base[group]) if base is not None and group in base else {}
        rows = []
        for c, r in cases:                                   # (consecutive cases with the same outcome share a line)
            if base is None or ref.get(c) != r:
                t = names.text(r)
                if rows and rows[-1][1] == t:
                    rows[-1][0].append(c)
                else:
                    rows.append(([c], t))
            else:
                rows.append(([], None))                      # (an equal case in between ends a run)
        rows = ['  %s %s' % (','.join(cs), t) for cs, t in rows if cs]
        if rows or base is None:
            lines += ['# ' + group] + rows
    return lines


def digest_section(res, names, base):
    lines = []
    for group, cases in res.items():
        ref = dict(base[group])
        n = sum(1 for c, r in cases if ref.get(c) != r)
        if n:
            h = hashlib.sha1('\n'.join('%s %s' % (c, names.text(r)) for c, r in cases).encode()).hexdigest()[:12]
            lines.append('# %s: %d of %d differ, %s' % (group, n, len(cases), h))
    return lines


def summarise(text):
    """The outline of an output, short enough to read in a diff: the size and digest of the two tables, then per section and entry
    point (the C function a group's name starts with; a knob section as a whole) the number of lines and a digest of them."""
    sections, entry = [('tables', {})], ''                   # [(title, {entry: lines})], dicts in order of appearance
    for line in text.rstrip('\n').split('\n'):
        if line.startswith('== '):
            sections.append((line[3:], {}))
            entry = ''
            continue
        title, blocks = sections[-1]
        if line.startswith('# ') and title != 'tables' and not title.startswith('SONET_'):
            entry = line[2:].split(' ')[0]
        blocks.setdefault(entry, []).append(line)
    out = []
    for title, blocks in sections:
        out.append('== ' + title)
        for entry, lines in blocks.items():
            out.append('  %s%d lines, %s' % (entry + ': ' if entry else '', len(lines), hashlib.sha1('\n'.join(lines).encode()).hexdigest()[:12]))
    return '\n'.join(out) + '\n'


def main():
    flags = {a for a in sys.argv[1:] if a.startswith('--')}
    args = [a for a in sys.argv[1:] if not a.startswith('--')]
    tree, variants, full, sanitize = os.path.abspath(args[0]), '--variants' in flags, '--full' in flags, '--sanitize' in flags
    with tempfile.TemporaryDirectory() as tmp:
        exe = build(tree, variants, sanitize, tmp)
        sections = []                                        # (title, run, reference run or None, digest only)
        base = run(exe, {})
        if variants:
            product = build(tree, False, sanitize, tmp)
            sections.append(('base, where it differs from the product build', base, run(product, {}), False))
            for knob, values, prefixes in KNOBS:
                for v in values:
                    sections.append(('%s=%s' % (knob, v), run(exe, {knob: v}, prefixes), base, not full))
            for knob, v, prefixes in KNOBS_X_CUS:
                for cus in CUS:
                    sections.append(('%s=%s LAUNCH_LOG_CUS=%s' % (knob, v, cus), run(exe, {knob: v, 'LAUNCH_LOG_CUS': cus}, prefixes), base, not full))
        else:
            sections.append(('base', base, None, False))
            for cus in CUS:
                sections.append(('LAUNCH_LOG_CUS=' + cus, run(exe, {'LAUNCH_LOG_CUS': cus}), base, False))
        # the second half (--bn): the family of the BatchNorm / ReLU passes, with tables of its own (appended to a recording that had none)
        bn = run(exe, {}, ['@bn']) if '--bn' in flags else None
        bn_sections = []
        if bn is None:
            pass
        elif variants:
            bn_sections.append(('bn passes: base, where it differs from the product build', bn, run(product, {}, ['@bn']), False))
            for knob, values, prefixes in BN_KNOBS:
                for v in values:
                    bn_sections.append(('bn passes: %s=%s' % (knob, v), run(exe, {knob: v}, ['@bn'] + prefixes), bn, False))   # (always in full: a digest hangs on table indices)
        else:
            bn_sections.append(('bn passes: base', bn, None, False))
        # the third half (--upconv): the decoder's up-convolutions.  The family reads no knob and asks for no CU count: the variants
        # build gets the half only where its text differs from the product build's
        up = run(exe, {}, ['@upconv']) if '--upconv' in flags else None
        up_sections = []
        if up is not None and not variants:
            up_sections.append(('upconv: base', up, None, False))
        elif up is not None and up != run(product, {}, ['@upconv']):
            up_sections.append(('upconv: base, where it differs from the product build', up, run(product, {}, ['@upconv']), False))
    out = []
    halves = [(None, sections)] + [(h, s) for h, s in (('bn passes: kernels and refusal texts', bn_sections), ('upconv: kernels and refusal texts', up_sections)) if s]
    for head, secs in halves:
        names = Names([s[1] for s in secs] + [s[2] for s in secs if s[2] is not None])
        out += ([] if head is None else ['== ' + head]) + ['K%d %s' % (i, n) for i, n in enumerate(names.table)] + ['E%d %s' % (i, n) for i, n in enumerate(names.errors)]
        for title, res, ref, digest in secs:
            out.append('== ' + title)
            out += digest_section(res, names, ref) if digest else full_section(res, names, ref)
    text = '\n'.join(out) + '\n'
    sys.stdout.write(summarise(text) if '--summary' in flags else text)
    return 0


if __name__ == '__main__':
    sys.exit(main())
