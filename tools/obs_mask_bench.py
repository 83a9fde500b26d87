"""What observation weights (partially observed labels: gpi_rom_desc.y_weight, gpi_rom_fit_desc.y_weight) cost,
and that they cost a launch without weights nothing.

--parent DIR is a checkout of the parent commit with its library built.  Two checkouts cannot share a process, so
every arm that compares them is a fresh child process per checkout and repeat, started alternately by this
process, which never touches the GPU.  Method everywhere: HIP events around graph replays (200 launches per
graph), arms interleaved, median with min - max of `--repeats` (9) timings.

 1. unweighted GPI_ROM_LOGLIK launch, N = 32 at 64^2 (nc = 8) and at 128^2 (nc = 16): this checkout beside the
    parent; this checkout's median must lie inside the parent's min - max spread.
 2. the same launch with 30 % observed, one shared row and per-sample rows, beside the unweighted launch (this
    checkout, the three arms interleaved in children of their own).  Reported, no bar.
 3. bench.py --gpus 1 --steps 200 --warmup 50 --dump-outputs in both checkouts: params, grad, adam_m, adam_v,
    elbo equal bit for bit; ms per step inside the parent's spread.
 4. gpi_rom_fit, T = 300, 64^2, N = 32: unweighted, with a quarter-density sensor grid, and the module-path loop
    (OptimizeEffectiveProperties with a plain column-selecting callable: what such a user ran before).

    python tools/obs_mask_bench.py --parent DIR [--out profiles/obs_mask_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LAUNCHES = 200
SHAPES = [('c64_nc8_N32', 8, 8, 32), ('c128_nc16_N32', 16, 8, 32)]


def _paths(root):
    for p in (root, os.path.join(root, 'generative-physics-informed-pde_amd')):
        if p not in sys.path:
            sys.path.insert(0, p)


def stats(v, nd=4):
    return dict(median=round(statistics.median(v), nd), min=round(min(v), nd), max=round(max(v), nd), repeats=len(v))


def graph_us(launch, stream, launches=LAUNCHES):
    """A graph of `launches` launches; returns a function that times one replay, us per launch."""
    import torch
    with torch.cuda.stream(stream):
        for _ in range(3):
            launch()
        stream.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            for _ in range(launches):
                launch()
        g.replay()
        stream.synchronize()

    def once():
        with torch.cuda.stream(stream):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            g.replay()
            e1.record(stream)
            e1.synchronize()
        return 1e3 * e0.elapsed_time(e1) / launches
    return once


def worker_rom(weighted):
    """One timing of every LOGLIK arm in this fresh process (the checkout on sys.path): us per launch."""
    import numpy as np
    import torch
    from gpi import _lib as L
    dev = torch.device('cuda', 0)
    s = torch.cuda.Stream()
    arms, keep = {}, []
    for name, nc, r, N in SHAPES:
        rng = np.random.default_rng(N + nc)
        n = nc * r
        dy, nn, nt = (n + 1) * (n - 1), (nc + 1) ** 2, 2 * nc * nc
        t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32, device=dev)
        x = t(rng.normal(0.3, 0.7, (N, nt)))
        F = np.zeros((N, nn), dtype=np.float32)
        bn = [e for e in range(nn) if e % (nc + 1) in (0, nc)]
        F[:, bn] = rng.uniform(-0.5, 0.5, (N, len(bn)))
        F, Y, ls = t(F), t(0.3 * rng.normal(size=(N, dy))), t(np.log(0.3) + 0.1 * rng.normal(size=dy))
        gx, part = torch.zeros_like(x), torch.empty(N, dy, device=dev)
        acc = torch.zeros(L.GPI_REPLICAS, dtype=torch.float64, device=dev)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        w = t(rng.random((N, dy)) < 0.3)
        keep += [x, F, Y, ls, gx, part, acc, flag, w]
        for arm in ('none', 'shared', 'per_sample') if weighted else ('none',):
            d = L.RomDesc()
            d.nc, d.refine, d.n, d.mode = nc, r, N, L.ROM_LOGLIK
            d.x, d.x_stride, d.F, d.Y, d.logsig_y = x.data_ptr(), nt, F.data_ptr(), Y.data_ptr(), ls.data_ptr()
            d.gx, d.gx_stride, d.gls_part, d.loss_acc, d.flag = (gx.data_ptr(), nt, part.data_ptr(), acc.data_ptr(),
                                                                flag.data_ptr())
            d.loss_scale = 1.0
            if arm != 'none':
                d.y_weight, d.yw_stride = w.data_ptr(), dy if arm == 'per_sample' else 0
            keep.append(d)
            fn = L.lib().gpi_rom
            launch = lambda d=d, fn=fn: L.check(fn(C.byref(d), L.stream_handle()), 'rom')
            arms[name + ':' + arm] = graph_us(launch, s)
    out = {k: [] for k in arms}
    for _ in range(3):                                            # interleaved; the child reports its medians
        for k, once in arms.items():
            out[k].append(once())
    print('RESULT ' + json.dumps({k: statistics.median(v) for k, v in out.items()}), flush=True)


def worker_fit(repeats):
    """gpi_rom_fit T = 300 at 64^2, N = 32: ms per fit, arms interleaved."""
    import numpy as np
    import torch
    from bottleneck.utils import OptimizeEffectiveProperties, ObservedDofs
    from bottleneck.ROM import ROM
    from bottleneck.components import ReducedOrderModelOperator
    from physics.grid import StructuredGrid
    from gpi.romfit import fit_effective_properties
    from oracle import fem
    dev = torch.device('cuda', 0)
    nc, r, N, T = 8, 8, 32, 300
    n = nc * r
    rng = np.random.default_rng(5)
    W = fem.prolongation_free(fem.unit_square_mesh(nc), fem.unit_square_mesh(n))
    mc = fem.unit_square_mesh(nc)
    F = torch.tensor(np.stack([fem.f_rom_bc(mc, u) for u in rng.uniform(-0.5, 0.5, (N, 4))]), dtype=torch.float32, device=dev)
    Y = torch.tensor(0.3 * rng.normal(size=(N, W.shape[0])), dtype=torch.float32, device=dev)
    idx = np.array([j * (n - 1) + (i - 1) for j in range(0, n + 1, 2) for i in range(1, n, 2)])
    obs = ObservedDofs(idx)
    g = ReducedOrderModelOperator(ROM(StructuredGrid(nc), r), torch.tensor(W, dtype=torch.float32), dtype=torch.float32,
                                  device='cuda')

    class DS(object):
        def get(self, k, **_):
            return {'Y': Y, 'F_ROM_BC': F}[k]

    idx_t = torch.tensor(idx, device=dev)
    arms = {'fit_unweighted': lambda: fit_effective_properties(Y, F, nc, r, T),
            'fit_sensor_grid': lambda: fit_effective_properties(Y, F, nc, r, T, y_weight=obs),
            'module_loop_sensor_grid': lambda: OptimizeEffectiveProperties(DS(), g, num_iterations=T, verbose=False,
                                                                           y_preprocessor=lambda y: y[..., idx_t])}
    ms = {k: [] for k in arms}
    for k, fn in arms.items():
        fn()
    for _ in range(repeats):
        for k, fn in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    print('RESULT ' + json.dumps(dict(nc=nc, refine=r, N=N, T=T, sensors=len(idx), d_y=int(W.shape[0]),
                                      ms_per_fit={k: stats(v) for k, v in ms.items()})), flush=True)


def child(root, args, timeout=900):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), '--root', root] + args, capture_output=True, text=True,
                       timeout=timeout)
    if r.returncode != 0:
        raise SystemExit('child %s in %s failed (%d):\n%s\n%s' % (args, root, r.returncode, r.stdout[-2000:], r.stderr[-4000:]))
    return json.loads([l for l in r.stdout.splitlines() if l.startswith('RESULT ')][-1][7:])


def bench_child(root, out_dir):
    """bench.py of a checkout (its own process tree), -> (ms per step, {name: array})."""
    import numpy as np
    r = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--gpus', '1', '--steps', '200', '--warmup', '50',
                        '--dump-outputs', out_dir], capture_output=True, text=True, timeout=900, cwd=root)
    if r.returncode != 0:
        raise SystemExit('bench.py in %s failed (%d):\n%s' % (root, r.returncode, r.stderr[-4000:]))
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith('{')][-1])
    arrays = {k: np.load(os.path.join(out_dir, k + '.npy')) for k in ('params', 'grad', 'adam_m', 'adam_v', 'elbo')}
    return line['ms_per_step'], arrays


def inside(this, parent):
    return bool(parent['min'] <= this['median'] <= parent['max'])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent', default=None)
    ap.add_argument('--repeats', type=int, default=9)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'obs_mask_bench.json'))
    ap.add_argument('--root', default=ROOT)
    ap.add_argument('--worker', choices=['rom', 'rom_weighted', 'fit'])
    ap.add_argument('--skip', default='', help='comma list of: rom, bench, fit')
    a = ap.parse_args()
    if a.worker:
        _paths(a.root)
        if a.worker == 'fit':
            return worker_fit(a.repeats)
        return worker_rom(a.worker == 'rom_weighted')
    skip = set(filter(None, a.skip.split(',')))
    parent = os.path.abspath(a.parent) if a.parent else None
    res = dict(method='HIP events around graph replays (%d launches per graph), arms interleaved, fresh child processes '
                      'alternated between the checkouts; median with min - max of the repeats' % LAUNCHES,
               repeats=a.repeats)
    if 'rom' not in skip:
        # the guard's two arms run the same worker (the unweighted launches alone); the weighted launches beside
        # the unweighted one in children of their own
        runs = {'this': [], 'parent': [], 'weighted': []}
        for i in range(a.repeats):
            if parent:
                runs['parent'].append(child(parent, ['--worker', 'rom']))
            runs['this'].append(child(ROOT, ['--worker', 'rom']))
            runs['weighted'].append(child(ROOT, ['--worker', 'rom_weighted']))
            print(i, runs['this'][-1], runs['parent'][-1] if parent else None, runs['weighted'][-1], flush=True)
        rom = {}
        for name, nc, r, N in SHAPES:
            e = dict(nc=nc, refine=r, N=N, this_none_us=stats([c[name + ':none'] for c in runs['this']], 3))
            e['weighted_run_us'] = {arm: stats([c[name + ':' + arm] for c in runs['weighted']], 3)
                                    for arm in ('none', 'shared', 'per_sample')}
            if parent:
                e['parent_none_us'] = stats([c[name + ':none'] for c in runs['parent']], 3)
                e['unweighted_inside_parent_spread'] = inside(e['this_none_us'], e['parent_none_us'])
            rom[name] = e
            print(name, e, flush=True)
        res['rom_loglik'] = rom
    if 'bench' not in skip and parent:
        import numpy as np
        ms = {'this': [], 'parent': []}
        equal = None
        with tempfile.TemporaryDirectory() as tmp:
            for i in range(a.repeats):
                pm, pa = bench_child(parent, os.path.join(tmp, 'p'))
                tm, ta = bench_child(ROOT, os.path.join(tmp, 't'))
                ms['parent'].append(pm)
                ms['this'].append(tm)
                eq = {k: bool(pa[k].shape == ta[k].shape and np.array_equal(pa[k].view(np.uint8), ta[k].view(np.uint8)))
                      for k in pa}
                equal = eq if equal is None else {k: equal[k] and eq[k] for k in eq}
                print(i, pm, tm, eq, flush=True)
        b = dict(this_ms_per_step=stats(ms['this']), parent_ms_per_step=stats(ms['parent']), bit_equal=equal)
        b['inside_parent_spread'] = inside(b['this_ms_per_step'], b['parent_ms_per_step'])
        res['bench_default_step'] = b
        print('bench', b, flush=True)
    if 'fit' not in skip:
        res['rom_fit'] = child(ROOT, ['--worker', 'fit', '--repeats', str(a.repeats)])
        print('fit', res['rom_fit'], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    if skip and os.path.exists(a.out):                # a run of some parts keeps the other parts' record
        with open(a.out) as fh:
            res = dict(json.load(fh), **res)
    with open(a.out, 'w') as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
        fh.write('\n')
    print('wrote', a.out)


if __name__ == '__main__':
    main()
