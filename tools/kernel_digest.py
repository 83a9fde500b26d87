"""Per-kernel digests of the gfx950 code in built objects (host only, no GPU): for every kernel the sha1 of its
machine code, its size and its VGPR / SGPR / spill counts -- the proof that a source change left a kernel's code
alone.  The device code object is taken out of the host object as tools/kernel_resources.sh does
(llvm-objdump --offloading); a kernel's bytes are [st_value, st_value + st_size) of its FUNC symbol in .text.  The
code objects carry no relocations (checked), so equal bytes are equal code wherever the kernel is loaded.

usage: python tools/kernel_digest.py OBJECT.o ...
           one line per kernel: sha1 size vgpr sgpr spill name
       python tools/kernel_digest.py --compare DIR_A DIR_B [--rename REGEX REPL] [OBJECT.o ...]
           the named objects (default conv.o conv_p1.o conv_p2.o conv_p3.o) of two build directories: per-object
           kernel counts, the kernels only in A / only in B and the kernels whose code differs, with the resource
           counts of both sides.  --rename rewrites A's mangled names (re.sub) before they are matched with B's,
           for a change that drops or adds a template argument.  Exit status 1 when a kernel present on both
           sides differs."""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get('ROCM_PATH', '/opt/rocm'), 'lib', 'llvm', 'bin')
DEFAULT_OBJECTS = ['conv.o', 'conv_p1.o', 'conv_p2.o', 'conv_p3.o']


def tool(name, *args, cwd=None):
    return subprocess.run([os.path.join(LLVM, name)] + list(args), cwd=cwd, check=True, stdout=subprocess.PIPE,
                          universal_newlines=True).stdout


def code_object(obj, tmp):
    """the gfx950 code object embedded in a host object, extracted into tmp"""
    link = os.path.join(tmp, 'k.o')
    if os.path.lexists(link):
        os.remove(link)
    os.symlink(os.path.abspath(obj), link)
    for f in os.listdir(tmp):
        if f.startswith('k.o.'):
            os.remove(os.path.join(tmp, f))
    tool('llvm-objdump', '--offloading', 'k.o', cwd=tmp)
    found = [f for f in os.listdir(tmp) if f.startswith('k.o.') and f.endswith('gfx950')]
    if len(found) != 1:
        raise SystemExit('%s: %d gfx950 code objects' % (obj, len(found)))
    return os.path.join(tmp, found[0])


def resources(co):
    """{kernel name: (vgpr, sgpr, spilled vgpr)} from the code object's metadata note"""
    res, name, cur = {}, None, {}
    for line in tool('llvm-readelf', '--notes', co).splitlines():
        m = re.match(r'\s+-?\s*\.(name|sgpr_count|vgpr_count|vgpr_spill_count):\s+(\S+)', line)
        if not m:
            continue
        if m.group(1) == 'name':
            name = m.group(2)
        else:
            cur[m.group(1)] = int(m.group(2))
        if m.group(1) == 'vgpr_spill_count':      # the last of a kernel's fields (sorted keys)
            res[name] = (cur['vgpr_count'], cur['sgpr_count'], cur['vgpr_spill_count'])
            cur = {}
    return res


def digests(obj, tmp):
    """{kernel name: (sha1, size, vgpr, sgpr, spill)} of one object"""
    co = code_object(obj, tmp)
    if re.search(r"^Relocation section", tool('llvm-readelf', '-r', co), re.M):
        raise SystemExit('%s: the code object has relocations; its bytes are not position independent' % obj)
    text = None
    for line in tool('llvm-readelf', '-S', '-W', co).splitlines():
        m = re.match(r'\s*\[\s*(\d+)\]\s+\.text\s+PROGBITS\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)', line)
        if m:
            text = (m.group(1), int(m.group(2), 16), int(m.group(3), 16), int(m.group(4), 16))
    if text is None:
        raise SystemExit('%s: no .text' % obj)
    ndx, addr, off, size = text
    data = open(co, 'rb').read()
    res = resources(co)
    out, in_symtab = {}, False
    for line in tool('llvm-readelf', '-s', '-W', co).splitlines():
        if line.startswith('Symbol table'):
            in_symtab = "'.symtab'" in line       # (-s lists .dynsym as well: each symbol once)
            continue
        f = line.split()
        if not in_symtab or len(f) != 8 or f[3] != 'FUNC' or f[6] != ndx:
            continue
        value, sz, name = int(f[1], 16), int(f[2]), f[7]
        if name not in res:
            continue                               # a device function, not a kernel
        if value < addr or value + sz > addr + size:
            raise SystemExit('%s: %s outside .text' % (obj, name))
        code = data[off + value - addr: off + value - addr + sz]
        out[name] = (hashlib.sha1(code).hexdigest(), sz) + res[name]
    if set(out) != set(res):
        raise SystemExit('%s: %d kernels in the metadata, %d FUNC symbols' % (obj, len(res), len(out)))
    return out


def fmt(name, d):
    return '%s %6d vgpr %3d sgpr %3d spill %3d  %s' % (d[0], d[1], d[2], d[3], d[4], name)


def compare(dir_a, dir_b, objects, rename):
    differs = 0
    with tempfile.TemporaryDirectory() as tmp:
        for o in objects:
            a = digests(os.path.join(dir_a, o), tmp)
            b = digests(os.path.join(dir_b, o), tmp)
            if rename:
                a = {re.sub(rename[0], rename[1], n): d for n, d in a.items()}
            only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
            diff = sorted(n for n in set(a) & set(b) if a[n][:2] != b[n][:2])
            print('%s: A %d kernels, B %d kernels, %d in both, %d of them with identical code' %
                  (o, len(a), len(b), len(set(a) & set(b)), len(set(a) & set(b)) - len(diff)))
            for title, names, side in (('only in A', only_a, a), ('only in B', only_b, b)):
                print('  %s: %d' % (title, len(names)))
                for n in names:
                    print('    ' + fmt(n, side[n]))
            print('  code differs: %d' % len(diff))
            for n in diff:
                print('    A ' + fmt(n, a[n]))
                print('    B ' + fmt(n, b[n]))
            differs += len(diff)
    return differs


def main():
    args = sys.argv[1:]
    if not args or args[0] in ('-h', '--help'):
        raise SystemExit(__doc__)
    if args[0] == '--compare':
        dir_a, dir_b, rest = args[1], args[2], args[3:]
        rename = None
        if rest[:1] == ['--rename']:
            rename, rest = (rest[1], rest[2]), rest[3:]
        sys.exit(1 if compare(dir_a, dir_b, rest or DEFAULT_OBJECTS, rename) else 0)
    with tempfile.TemporaryDirectory() as tmp:
        for o in args:
            d = digests(o, tmp)
            print('# %s: %d kernels' % (o, len(d)))
            for n in sorted(d):
                print(fmt(n, d[n]))


if __name__ == '__main__':
    main()
