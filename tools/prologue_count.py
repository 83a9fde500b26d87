"""Static instruction counts of the conv kernels' prologues (host only, no GPU): for every kernel of the given
objects whose demangled name matches a regex, the VALU / SALU / VMEM / LDS-DMA / DS instructions in program order
before the first s_barrier (the operand staging and everything else a workgroup issues before it first waits), and
the exec-mask saves among them (a branch the compiler put around a load, or a loop around a buffer access with a
descriptor it could not prove uniform).

usage: python tools/prologue_count.py [--match REGEX] OBJECT.o ...
       python tools/prologue_count.py --compare DIR_A DIR_B [--match REGEX] [OBJECT.o ...]   (default conv.o)
"""
import os
import re
import shutil
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_digest import LLVM, code_object, resources  # noqa: E402

KEYS = ('valu', 'salu', 'vmem', 'dma', 'ds', 'saveexec', 'total')


def classify(op):
    if op.startswith('v_'):
        return 'valu'
    if op.startswith(('buffer_', 'global_', 'flat_', 'scratch_')):
        return 'vmem'
    if op.startswith('ds_'):
        return 'ds'
    if op.startswith('s_'):
        return 'salu'
    return None


def counts(obj, tmp, match):
    co = code_object(obj, tmp)
    kernels = set(resources(co))
    dis = subprocess.run([os.path.join(LLVM, 'llvm-objdump'), '-d', '--no-show-raw-insn', co], check=True,
                         stdout=subprocess.PIPE, universal_newlines=True).stdout
    nice = {n: n for n in kernels}
    filt = shutil.which('c++filt') or shutil.which('llvm-cxxfilt', path=LLVM)
    if filt:                                 # demangled names where a demangler is installed
        names = subprocess.run([filt], input='\n'.join(sorted(kernels)), check=True, stdout=subprocess.PIPE,
                               universal_newlines=True).stdout.splitlines()
        nice = dict(zip(sorted(kernels), names))
    out, cur, done = {}, None, False
    for line in dis.splitlines():
        m = re.match(r'^[0-9a-f]+ <(\S+)>:', line)
        if m:
            name = m.group(1)
            cur = None
            if name in kernels and re.search(match, nice[name]):
                cur = out.setdefault(name, dict.fromkeys(KEYS, 0))
                done = False
            continue
        if cur is None or done:
            continue
        f = line.split()
        if not f:
            continue
        op = f[0]
        if op == 's_barrier':
            done = True
            continue
        k = classify(op)
        if k is None:
            continue
        cur[k] += 1
        cur['total'] += 1
        if ' lds' in line and k == 'vmem':
            cur['dma'] += 1
        if 'saveexec' in op:
            cur['saveexec'] += 1
    return out, nice


def short(n):
    n = re.sub(r'^void \(anonymous namespace\)::', '', n)
    return n.split('(')[0]


def main():
    args = sys.argv[1:]
    if not args or args[0] in ('-h', '--help'):
        raise SystemExit(__doc__)
    compare = args[0] == '--compare'
    if compare:
        dirs, args = args[1:3], args[3:]
    match = '.'
    if args[:1] == ['--match']:
        match, args = args[1], args[2:]
    objs = args or ['conv.o']
    with tempfile.TemporaryDirectory() as tmp:
        for o in objs:
            if not compare:
                c, nice = counts(o, tmp, match)
                print('# %s: %d kernels; before the first s_barrier: %s' % (o, len(c), ' '.join(KEYS)))
                for n in sorted(c, key=lambda n: nice[n]):
                    print(' '.join('%5d' % c[n][k] for k in KEYS) + '  ' + short(nice[n]))
                continue
            a, nice = counts(os.path.join(dirs[0], o), tmp, match)
            b, nice_b = counts(os.path.join(dirs[1], o), tmp, match)
            nice.update(nice_b)
            both = sorted(set(a) & set(b), key=lambda n: nice[n])
            print('# %s: %d kernels on both sides; before the first s_barrier, A -> B: %s' % (o, len(both), ' '.join(KEYS)))
            for n in both:
                print(' '.join('%4d->%4d' % (a[n][k], b[n][k]) for k in KEYS) + '  ' + short(nice[n]))
            for k in KEYS:
                sa, sb = sum(a[n][k] for n in both), sum(b[n][k] for n in both)
                print('# sum %-8s %7d -> %7d (%+.1f %%)' % (k, sa, sb, 100.0 * (sb - sa) / max(sa, 1)))


if __name__ == '__main__':
    main()
