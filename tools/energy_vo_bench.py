"""Cost of one energy virtual-observable update (EnergyVirtualObservablesEnsemble.update, gpi_vo_energy).

Shapes (m_aux = 8 RBF test functions, n_iter = 10 inner iterations per update, as --m-aux / --n-iter):
  64 x 64,   N = 128 VO samples   the bench grid: FUSED form (one workgroup per sample, one launch)
  128 x 128, N = 32               TILED form (three launches per inner iteration)
On the GPU each timed block is a host clock around `--calls` updates ending in a device synchronise, after a
dropped warm-up block; reported: median and min..max over `--rounds` blocks, the time per inner iteration,
and the share of a training iteration an update costs when it runs every `--interval` steps (the reference
trainer's N_vo_update_interval, 250 by default) next to a training step of `--step-ms` (default: bench.py's
recorded 64 x 64 step).

The stated baseline is other hardware: the fp64 numpy restatement of the reference's update
(VirtualObservables.py:769-788: dense A = diag(prec) + K / T per sample, V^T A V and the solve per inner
iteration) on this host's cores (`--host-threads`, 16 by default), `--host-samples` samples per shape scaled to N.
`--part gpu` / `--part host` measure one side only and update the --out file, so the two can run apart.

    python tools/energy_vo_bench.py --out profiles/energy_vo_bench.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'generative-physics-informed-pde_amd'))

SHAPES = [(64, 128), (128, 32)]


def block_ms(fn, calls, sync):
    sync()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    sync()
    return (time.perf_counter() - t0) * 1e3 / calls


def summary(xs):
    return {'median_ms': statistics.median(xs), 'min_ms': min(xs), 'max_ms': max(xs), 'blocks': len(xs)}


def host_update_ms(n, m_aux, n_iter, length, samples, rng):
    """The reference's update of one sample in fp64 numpy, dense as the reference runs it; ms per sample."""
    import numpy as np
    from oracle import fem
    mf = fem.unit_square_mesh(n)
    P = mf.coords[fem.dirichlet_split(mf)[1]]
    dy = P.shape[0]
    times = []
    for _ in range(samples):
        K, f = fem.assemble_system(mf, np.exp(rng.normal(0.3, 0.9, 2 * n * n)), rng.uniform(-0.5, 0.5, 4))
        K, f = np.asarray(K), np.asarray(f).reshape(-1)
        prec = 1.0 / rng.uniform(0.01, 0.1, dy) ** 2
        g = rng.normal(0, 0.3, dy)
        mean = np.zeros(dy)
        t0 = time.perf_counter()
        beta = 1.0 / 0.5
        vars_ = 1.0 / (prec + beta * K.diagonal())                                    # noqa: F841
        A = np.diag(prec) + beta * K
        b = beta * f + prec * g
        for _it in range(n_iter):
            c = rng.uniform(0, 1, (m_aux, 2))
            V = np.exp(-((P[:, 0:1] - c[None, :, 0]) ** 2 + (P[:, 1:2] - c[None, :, 1]) ** 2) / length ** 2)
            M = V.T @ A @ V
            mean = mean - V @ np.linalg.solve(M, V.T @ (A @ mean - b))
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--m-aux', type=int, default=8)
    ap.add_argument('--n-iter', type=int, default=10)
    ap.add_argument('--length', type=float, default=0.1)
    ap.add_argument('--calls', type=int, default=20, help='updates per timed block')
    ap.add_argument('--rounds', type=int, default=7, help='timed blocks per shape')
    ap.add_argument('--interval', type=int, default=250, help='training steps between VO updates')
    ap.add_argument('--step-ms', type=float, default=0.4451, help='ms of one 64 x 64 training step (bench.py)')
    ap.add_argument('--host-threads', type=int, default=16)
    ap.add_argument('--host-samples', type=int, default=2)
    ap.add_argument('--part', choices=['all', 'gpu', 'host'], default='all',
                    help="which side to measure; an existing --out file is updated, so the host baseline can "
                         "run apart from the GPU")
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'energy_vo_bench.json'))
    a = ap.parse_args()
    for k in ('OMP_NUM_THREADS', 'OPENBLAS_NUM_THREADS', 'MKL_NUM_THREADS'):
        os.environ[k] = str(a.host_threads)
    import numpy as np
    rng = np.random.default_rng(0)
    res = {'shapes': {}}
    if os.path.exists(a.out):
        with open(a.out) as fh:
            res = json.load(fh)
    res.update(m_aux=a.m_aux, n_iter=a.n_iter, length=a.length, interval=a.interval, step_ms=a.step_ms)
    if a.part in ('all', 'gpu'):
        gpu_part(a, res, rng)
    if a.part in ('all', 'host'):
        res['host_threads'] = a.host_threads
        for n, N in SHAPES:
            out = res['shapes'].setdefault('%dx%d' % (n, n), {'N': N})
            host = host_update_ms(n, a.m_aux, a.n_iter, a.length, a.host_samples, rng)
            out['host_numpy_ms_per_sample'] = host
            out['host_numpy_ms'] = host * N
            print('%d x %d host numpy: %.1f ms per sample' % (n, n, host))
    for out in res['shapes'].values():
        if 'median_ms' in out and 'host_numpy_ms' in out:
            out['host_over_gpu'] = out['host_numpy_ms'] / out['median_ms']
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
        fh.write('\n')
    print('wrote', a.out)


def gpu_part(a, res, rng):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('energy_vo_bench needs a GPU for --part gpu / all: nothing is measured without one')
    from gpi import _lib as L
    from gpi.vo import vo_energy_form
    from bottleneck import VirtualObservables as VO
    from physics.LinearElliptic import LinearEllipticPhysics
    from physics.BoundaryConditions import BoundaryCondition
    dev = torch.device('cuda:0')
    sync = lambda: torch.cuda.synchronize(dev)
    torch.manual_seed(0)
    names = {L.VO_ENERGY_FUSED: 'fused', L.VO_ENERGY_TILED: 'tiled'}
    res.update(device=torch.cuda.get_device_name(0), calls_per_block=a.calls, rounds=a.rounds)
    for n, N in SHAPES:
        dy = (n + 1) * (n - 1)
        phys = LinearEllipticPhysics('fom', 'NDP', n)
        QPE = VO.QuerryPointEnsemble([VO.QuerryPoint(phys, rng.normal(0.3, 0.9, 2 * n * n),
                                                     BoundaryCondition(rng.uniform(-0.5, 0.5, 4))) for _ in range(N)])
        sampler = VO.RadialBasisFunctionSampler(QPE[0], l=a.length, N_aux=a.m_aux, device=dev)
        ens = VO.EnergyVirtualObservablesEnsemble(QPE, a.n_iter, sampler, dtype=torch.float32, device=dev)
        ens.force_temperature(0.5)
        G = torch.tensor(rng.normal(0, 0.3, (N, dy)), dtype=torch.float32, device=dev)
        PREC = torch.tensor(1.0 / rng.uniform(0.01, 0.1, (N, dy)) ** 2, dtype=torch.float32, device=dev)
        upd = lambda: ens.update(G, PREC, 0)
        blocks = [block_ms(upd, a.calls, sync) for _ in range(a.rounds + 1)][1:]       # block 0 warms up
        ens.check_flag()
        assert torch.isfinite(ens.mean64).all()
        out = res['shapes'].setdefault('%dx%d' % (n, n), {})
        out.update(summary(blocks))
        out['form'] = names[vo_energy_form(n, a.m_aux)]
        out['N'] = N
        out['per_iteration_ms'] = out['median_ms'] / a.n_iter
        out['share_of_training'] = out['median_ms'] / (a.interval * a.step_ms)
        print('%d x %d' % (n, n), json.dumps(out))


if __name__ == '__main__':
    main()
