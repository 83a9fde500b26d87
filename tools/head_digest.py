"""Bit digests and launch times of the dense head (csrc/head.hip) and the gp MLP (csrc/gpmlp.hip), to compare two
builds of the library.

Digests (default mode): one sha256 per output buffer -- every workspace region and every accumulator block of
tests/head_cases.py's 208 cases (the tool imports the table), each of the seven term sums' raw replica slots, the
whole accumulator, and the 81 bare gpi_outer_gemm cases' accumulators; for gpi_gpmlp_forward / _backward every
workspace buffer after each launch, the term slots and the accumulator, at 64-85-106-128 and 16-21-26-32 with two
segments (20 + 7 rows: the second tile holds both), free-X and lock-X (the Case of tests/test_gpu_gp_mlp.py).
The library and the GPI_HEAD_* switches are read once per process, so the driver runs every arm as a fresh child
(`--arm`), one after another, each under its own timeout, and stops at the first failure:
  libraries   parent, parent2: GPI_LIB_VARIANT=parent GPI_ALLOW_STALE_LIB=1 (libgpi_hip_parent.so, built from the
              parent's csrc: make -C csrc OUT=../gpi/libgpi_hip_parent.so BUILD=build_parent), twice;
              new: the library of this tree
  head arms   default (default dispatch), valu (GPI_HEAD_VALU and the scalar GEMM tiles), generic
              (GPI_HEAD_PREFETCH=0, the two family layouts), mfma_off (GPI_HEAD_MFMA=0); and gpmlp
A buffer whose digest agrees between the two parent arms must have that digest in the new arm.  A buffer the parent
does not repeat is listed, and is a failure unless it is an fp64 target that receives atomic adds from several
workgroups (term slots, logsigma_X's gradient, the whole accumulator; the variational rows under the VALU kernels):
those are left to the fp64 sweep of tests/test_gpu_head_ops.py.

    python tools/head_digest.py > profiles/head_refactor_digest.txt

Times (`--time`): HIP-event times of a captured graph of REPS x (gpi_head_forward, gpi_head_backward,
gpi_outer_gemm) at the bench step's head shape (80/64/64/128, 256 + 32 + 0 samples, free-X) in default dispatch
(prefetched family 1), in the generic MFMA form (GPI_HEAD_PREFETCH=0) and in the VALU form, at family 2's widths
(64/16/64/32), and of gpi_gpmlp_forward + _backward at L = 1 (64-96-128, 32 rows).  Parent and new alternate as fresh
processes after one discarded warm-up pair; the new library's median must lie inside the parent's min..max or below.

    python tools/head_digest.py --time --alternations 10
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'generative-physics-informed-pde_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

# head arm -> environment of the child
ARMS = [('default', {}), ('valu', {}), ('generic', {'GPI_HEAD_PREFETCH': '0'}), ('mfma_off', {'GPI_HEAD_MFMA': '0'}),
        ('gpmlp', {})]
SWITCHES = ('GPI_HEAD_PREFETCH', 'GPI_HEAD_MFMA', 'GPI_LIB_VARIANT', 'GPI_ALLOW_STALE_LIB')
GPMLP_WIDTHS = ([64, 85, 106, 128], [16, 21, 26, 32])
GPMLP_SEGS = [(20, 1.0), (7, 0.25)]
REPS = 10            # launches of each entry point per captured graph
REPLAYS = 100        # graph replays per timed window
WINDOWS = 5          # windows per figure (their median)


def sha(a):
    import numpy as np
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


class HeadRun:
    """One head case's device buffers; launch() enqueues forward, backward and the outer GEMM."""

    def __init__(self, case, valu, dev):
        import torch
        from gpi import _lib as L
        import head_cases as H
        self.L, self.lib, self.c = L, L.lib(), case
        self.P = torch.from_numpy(case.param_vector()).to(dev)
        self.ws = torch.from_numpy(case.workspace()).to(dev)
        self.gacc = torch.zeros(case.n_params, dtype=torch.float64, device=dev)
        self.terms = torch.zeros(7 * H.REPLICAS, dtype=torch.float64, device=dev)
        self.hd = case.desc(L, self.terms.data_ptr(), L.HEAD_VALU if valu else 0)
        self.items = case.gemm_items(L, valu)

    def launch(self):
        L, lib, st = self.L, self.lib, self.L.stream_handle()
        L.check(lib.gpi_head_forward(C.byref(self.hd), L.ptr(self.P), L.ptr(self.ws), st), 'head forward')
        L.check(lib.gpi_head_backward(C.byref(self.hd), L.ptr(self.P), L.ptr(self.ws), L.ptr(self.gacc), st),
                'head backward')
        if len(self.items):
            L.check(lib.gpi_outer_gemm(self.items, len(self.items), L.ptr(self.ws), L.ptr(self.gacc), st), 'outer gemm')


def head_child(arm):
    import torch
    import head_cases as H
    from gpi import _lib as L
    dev = torch.device('cuda:0')
    valu = arm == 'valu'
    layouts = H.FAMILY_LAYOUTS if arm == 'generic' else tuple(H.LAYOUTS)
    emit = lambda case, buf, a: print('DIGEST %s|%s %s' % (case, buf, sha(a)), flush=True)
    for layout in layouts:
        for c in H.layout_cases(layout):
            r = HeadRun(c, valu, dev)
            form = r.lib.gpi_head_form(C.byref(r.hd), 0 if arm == 'generic' else 1)
            r.launch()
            torch.cuda.synchronize()
            ws, gacc, terms = r.ws.cpu().numpy(), r.gacc.cpu().numpy(), r.terms.cpu().numpy()
            print('FORM %s %d' % (c.id, 0 if arm == 'mfma_off' else form))
            for k, reg in c.w_reg.items():
                emit(c.id, 'ws:' + k, reg.view(ws))
            for k, reg in c.p_reg.items():
                emit(c.id, 'grad:' + k, reg.view(gacc))
            for t in range(7):
                emit(c.id, 'terms:%d' % t, terms[t * H.REPLICAS:(t + 1) * H.REPLICAS])
            emit(c.id, 'acc', gacc)
    if arm != 'generic':
        for g in H.gemm_cases():
            ws = torch.from_numpy(g.ws).to(dev)
            gacc = torch.zeros(g.n_gacc, dtype=torch.float64, device=dev)
            items = g.gemm_items(L, valu)
            L.check(L.lib().gpi_outer_gemm(items, len(items), L.ptr(ws), L.ptr(gacc), L.stream_handle()), 'outer gemm')
            torch.cuda.synchronize()
            emit('gemm ' + g.id, 'acc', gacc.cpu().numpy())
    print('ARM OK', flush=True)


def gpmlp_case(widths, segs, lockx, dev):
    from test_gpu_gp_mlp import Case
    c = Case(widths, segs, lockx, seed=7)
    c.layout(dev)
    return c


def gpmlp_child():
    import torch
    dev = torch.device('cuda:0')
    for widths in GPMLP_WIDTHS:
        for lockx in (False, True):
            c = gpmlp_case(widths, GPMLP_SEGS, lockx, dev)
            tag = 'gpmlp %s %s' % ('-'.join(map(str, widths)), 'lockX' if lockx else 'freeX')
            ws_f, ws_b, terms, gacc = c.run(dev)
            edges = sorted(c.woff.items(), key=lambda kv: kv[1]) + [('end', c.wsz)]
            for (name, o), (_, o1) in zip(edges[:-1], edges[1:]):      # each buffer with the sentinel gap after it
                print('DIGEST %s|fwd ws:%s %s' % (tag, name, sha(ws_f[o:o1].numpy())))
                print('DIGEST %s|bwd ws:%s %s' % (tag, name, sha(ws_b[o:o1].numpy())))
            offs = sorted(c.off.items(), key=lambda kv: kv[1]) + [('end', gacc.numel())]
            for (name, o), (_, o1) in zip(offs[:-1], offs[1:]):
                print('DIGEST %s|grad:%s %s' % (tag, name, sha(gacc[o:o1].numpy())))
            print('DIGEST %s|terms %s' % (tag, sha(terms.numpy())))
            print('DIGEST %s|acc %s' % (tag, sha(gacc.numpy())))
    print('ARM OK', flush=True)


def time_graph(launch):
    """us per launch() from a captured graph of REPS launches: median of WINDOWS windows of REPLAYS replays"""
    import torch
    launch()                                            # (module load, lazy initialisation: outside the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(REPS):
            launch()
    for _ in range(20):
        g.replay()
    torch.cuda.synchronize()
    out = []
    for _ in range(WINDOWS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(REPLAYS):
            g.replay()
        b.record()
        b.synchronize()
        out.append(1e3 * a.elapsed_time(b) / (REPLAYS * REPS))
    return statistics.median(out)


def time_child(which):
    import torch
    import head_cases as H
    from gpi import _lib as L
    dev = torch.device('cuda:0')
    bench = lambda layout, valu: HeadRun(H.Case(0, layout, (256, 32, 0), 'freeX'), valu, dev)
    res = {}
    if which == 'generic':
        assert os.environ.get('GPI_HEAD_PREFETCH') == '0'
        r = bench('w80_64_64_128', False)
        assert r.lib.gpi_head_form(C.byref(r.hd), 0) == 1
        res['generic_80_64_64_128'] = time_graph(r.launch)
    else:
        for name, layout, valu, form in (('bench_80_64_64_128', 'w80_64_64_128', False, 2),
                                         ('family2_64_16_64_32', 'w64_16_64_32', False, 3),
                                         ('valu_80_64_64_128', 'w80_64_64_128', True, 0)):
            r = bench(layout, valu)
            assert r.lib.gpi_head_form(C.byref(r.hd), 1) == form, name
            res[name] = time_graph(r.launch)
        c = gpmlp_case([64, 96, 128], [(32, 1.0)], False, dev)
        ws, lib = c.ws0.to(dev), L.lib()
        gacc = torch.zeros(c.P.numel(), dtype=torch.float64, device=dev)

        def launch():
            st = L.stream_handle()
            L.check(lib.gpi_gpmlp_forward(C.byref(c.desc), L.ptr(c.P), L.ptr(ws), st), 'gpmlp forward')
            L.check(lib.gpi_gpmlp_backward(C.byref(c.desc), L.ptr(c.P), L.ptr(ws), L.ptr(gacc), st), 'gpmlp backward')
        res['gpmlp_64_96_128'] = time_graph(launch)
    print('TIME ' + json.dumps(res), flush=True)


def run_child(lib, args, extra, timeout):
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(extra)
    if lib != 'new':
        env.update(GPI_LIB_VARIANT='parent', GPI_ALLOW_STALE_LIB='1')
    cmd = ['timeout', '-k', '10', str(timeout), sys.executable, os.path.abspath(__file__)] + args
    r = subprocess.run(cmd, env=env, capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit('child %s %s failed (%d):\n%s\n%s' % (lib, args, r.returncode, r.stdout[-2000:], r.stderr[-4000:]))
    print('ran %s %s %s' % (lib, ' '.join(args), extra or ''), file=sys.stderr, flush=True)
    return r.stdout


def may_differ(arm, buf):
    """fp64 targets of atomic adds from several workgroups: the only buffers a library need not repeat"""
    if buf.startswith('terms') or buf in ('acc', 'grad:gp_ls'):
        return True
    return arm in ('valu', 'mfma_off') and buf.startswith('grad:q')


def digest_main(timeout):
    got, forms = {}, {}
    for lib in ('parent', 'parent2', 'new'):
        for arm, extra in ARMS:
            out = run_child(lib, ['--arm', arm], extra, timeout)
            if 'ARM OK' not in out:
                raise SystemExit('arm %s/%s did not finish:\n%s' % (lib, arm, out[-2000:]))
            got[lib, arm] = dict(l.split(' ', 1)[1].rsplit(' ', 1) for l in out.splitlines() if l.startswith('DIGEST '))
            forms[lib, arm] = [l for l in out.splitlines() if l.startswith('FORM ')]
    differ, must_repeat = [], []
    for arm, _ in ARMS:
        a, b, n = got['parent', arm], got['parent2', arm], got['new', arm]
        if not (set(a) == set(b) == set(n)) or not (forms['parent', arm] == forms['parent2', arm] == forms['new', arm]):
            raise SystemExit('arm %s: the libraries ran different cases or kernel forms' % arm)
        by_form = {}
        for l in forms['new', arm]:
            by_form[l.rsplit(' ', 1)[1]] = by_form.get(l.rsplit(' ', 1)[1], 0) + 1
        groups, listed, allowed = {}, [], {}
        for key in a:
            case, buf = key.split('|')
            g = case.split('-')[0] if not case.startswith(('gemm', 'gpmlp')) else case.split(' ')[0]
            s = groups.setdefault(g, [0, 0, 0, hashlib.sha256()])
            s[0] += 1
            s[3].update(n[key].encode())
            if a[key] != b[key]:
                s[1] += 1
                if may_differ(arm, buf):
                    allowed[buf] = allowed.get(buf, 0) + 1
                    continue
                must_repeat.append('%s %s' % (arm, key))
                listed.append('    not repeated by the parent: %-60s parent %s parent2 %s new %s' %
                              (key, a[key][:12], b[key][:12], n[key][:12]))
            elif n[key] != a[key]:
                s[2] += 1
                differ.append('%s %s' % (arm, key))
                listed.append('    DIFFERENT: %-60s parent %s new %s' % (key, a[key][:12], n[key][:12]))
        print('arm %-9s cases by kernel form %s' % (arm, dict(sorted(by_form.items())) or '-'))
        for g, (tot, unst, bad, h) in groups.items():
            print('  %-20s %5d buffers, %5d equal to the parent, %3d not repeated by the parent, %3d different'
                  '   (sha256 of the new digests %s)' % (g, tot, tot - unst - bad, unst, bad, h.hexdigest()[:16]))
        if allowed:
            print('    fp64 atomic targets the parent does not repeat (buffer: cases): %s' % dict(sorted(allowed.items())))
        print('\n'.join(listed) if listed else '    every repeatable buffer equal in the new library')
    if must_repeat:
        print('single-writer buffers the parent does not repeat (a finding): %s' % must_repeat)
    print('RESULT: %s' % ('every repeatable buffer has the parent\'s bits' if not (differ or must_repeat)
                          else 'DIFFERENT: %s' % (differ + ['(must repeat) ' + u for u in must_repeat])))
    return 1 if differ or must_repeat else 0


def time_main(alternations, timeout):
    def pair(lib):
        res = {}
        for which, extra in (('default', {}), ('generic', {'GPI_HEAD_PREFETCH': '0'})):
            out = run_child(lib, ['--arm', 'time', '--which', which], extra, timeout)
            res.update(json.loads([l for l in out.splitlines() if l.startswith('TIME ')][-1][5:]))
        return res
    for lib in ('parent', 'new'):
        pair(lib)                                       # warm-up, discarded
    runs = {'parent': [], 'new': []}
    for alt in range(alternations):
        for lib in (('parent', 'new') if alt % 2 == 0 else ('new', 'parent')):
            r = pair(lib)
            runs[lib].append(r)
            print('alternation %2d %-6s %s' % (alt + 1, lib, ' '.join('%s=%.3f' % kv for kv in sorted(r.items()))),
                  flush=True)
    bad = 0
    print('us per (forward + backward [+ outer GEMM]); %d alternations, first of each pair alternating' % alternations)
    for k in sorted(runs['parent'][0]):
        p, n = [r[k] for r in runs['parent']], [r[k] for r in runs['new']]
        med = statistics.median(n)
        verdict = 'inside' if min(p) <= med <= max(p) else ('below' if med < min(p) else 'ABOVE')
        bad += verdict == 'ABOVE'
        print('  %-22s parent %.3f..%.3f (median %.3f) | new %.3f..%.3f median %.3f   %s' %
              (k, min(p), max(p), statistics.median(p), min(n), max(n), med, verdict))
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--arm', help='child: default | valu | generic | mfma_off | gpmlp | time')
    ap.add_argument('--which', default='default', help='child --arm time: default | generic')
    ap.add_argument('--time', action='store_true', help='the timing comparison instead of the digests')
    ap.add_argument('--alternations', type=int, default=10)
    ap.add_argument('--timeout', type=int, default=180)
    a = ap.parse_args()
    if a.arm == 'time':
        return time_child(a.which)
    if a.arm == 'gpmlp':
        return gpmlp_child()
    if a.arm is not None:
        return head_child(a.arm)
    return time_main(a.alternations, a.timeout) if a.time else digest_main(a.timeout)


if __name__ == '__main__':
    sys.exit(main())
