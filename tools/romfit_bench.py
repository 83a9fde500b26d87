"""Cost of the optimal-effective-property fit (OptimizeEffectiveProperties, T = 300 Adam iterations).

Two arms on the same labels, interleaved in one process, each timed with HIP events around the whole fit
after a warm-up fit per shape and arm; reported: median (min..max) over `--repeats` fits.
  A  one gpi_rom_fit launch (gpi/romfit.py): one wave per sample, every iteration inside the kernel
  B  the module-path loop a user writes without it: RomOperatorFunction (gpi_rom FORWARD + BACKWARD) +
     mse_loss + torch.optim.Adam, T host-launched iterations
Shapes: 64 x 64 (nc = 8) with N = 32 and N = 2048; 128 x 128 (nc = 8) N = 512; 256 x 256 (nc = 8) N = 128;
32 x 32 (nc = 4) N = 128.  --set nc16: the 16 x 16 coarse mesh, 128 x 128 (refine 8) with N = 32 and N = 512,
256 x 256 (refine 16) N = 128, written to profiles/romfit16_bench.json.

Also reported from the shapes: the bytes arm A has to move (Y once, F, x / m / v in and out, the records) and
the useful flops of one iteration of one sample (band Cholesky, the 63 forward substitutions that form
Z = L^{-1}, four triangular mat-vecs, the 7-point fp64 G u; nc = 16: band Cholesky with the forward
substitution riding along and three band sweeps instead), which give the achieved bandwidth and flop rate
next to the time of one iteration of one wave -- the fit is a chain of dependent steps inside each wave
(latency-bound), not a bandwidth or throughput problem.

    python tools/romfit_bench.py --out profiles/romfit_bench.json
    python tools/romfit_bench.py --set nc16
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'generative-physics-informed-pde_amd'))

SHAPES = {'nc8': [(64, 8, 32), (64, 8, 2048), (128, 8, 512), (256, 8, 128), (32, 4, 128)],   # (n_fine, nc, N)
          'nc16': [(128, 16, 32), (128, 16, 512), (256, 16, 128)]}
OUT = {'nc8': 'romfit_bench.json', 'nc16': 'romfit16_bench.json'}


def summary(xs):
    return {'median_ms': statistics.median(xs), 'min_ms': min(xs), 'max_ms': max(xs), 'repeats': len(xs)}


def algorithmic(n, nc, N, T):
    """(bytes arm A moves, useful flops per iteration per sample)."""
    dy, nn, nt, ni, bw = (n + 1) * (n - 1), (nc + 1) ** 2, 2 * nc * nc, (nc - 1) * (nc + 1), nc - 1
    nbytes = 4 * N * dy + 4 * N * nn + 2 * 3 * 4 * N * nt + 8 * T * N + 8 * N + 4 * N * nt + 4 * N * nn
    chol = ni * (bw + bw * (bw + 1))                    # scale the column, rank-1 update of the window (fma = 2)
    zform = 2 * bw * ni * (ni + 1) // 2                 # forward substitution of e_j, j < NI
    matvec = 4 * ni * (ni + 1)                          # four triangular mat-vecs, fma = 2
    if nc == 16:                                        # no Z: four band substitutions (one inside the factorisation)
        zform, matvec = 0, 4 * ni * (2 * bw + 1)
    rest = 2 * 7 * nn + 3 * nn + 12 * nt + 20 * nt      # G u and ss (fp64), the edge formula, exp + Adam
    return nbytes, chol + zform + matvec + rest


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=300)
    ap.add_argument('--lr', type=float, default=1e-2)
    ap.add_argument('--repeats', type=int, default=9)
    ap.add_argument('--set', choices=sorted(SHAPES), default='nc8')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    a.out = a.out or os.path.join(ROOT, 'profiles', OUT[a.set])
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('romfit_bench needs a GPU: nothing is measured without one')
    from gpi.native import RomOperatorFunction
    from gpi.romfit import fit_effective_properties
    from oracle import fem
    dev = torch.device('cuda:0')
    T = a.iters
    res = {'device': torch.cuda.get_device_name(0), 'iters': T, 'lr': a.lr, 'shapes': {}}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for n, nc, N in SHAPES[a.set]:
        r = n // nc
        rng = np.random.default_rng(n + N)
        mc = fem.unit_square_mesh(nc)
        F = torch.tensor(np.stack([fem.f_rom_bc(mc, u) for u in rng.uniform(-0.5, 0.5, (N, 4))]), dtype=torch.float32,
                         device=dev)
        xs = torch.tensor(0.7 * rng.standard_normal((N, 2 * nc * nc)), dtype=torch.float32, device=dev)
        mu, _ = RomOperatorFunction.apply(xs, F, nc, r, False)
        Y = mu + 0.05 * torch.randn(mu.shape, device=dev, generator=torch.Generator(dev).manual_seed(n + N))

        last = {}

        def arm_a():
            last['a'] = fit_effective_properties(Y, F, nc, r, T, lr=a.lr)

        def arm_b():
            x = torch.zeros(N, 2 * nc * nc, device=dev, requires_grad=True)
            opt = torch.optim.Adam([x], lr=a.lr)
            for _ in range(T):
                pred, _ = RomOperatorFunction.apply(x, F, nc, r, False)
                J = torch.nn.functional.mse_loss(pred, Y)
                opt.zero_grad()
                J.backward()
                opt.step()
            last['b'] = (x.detach(), J.detach())

        timed(arm_a)                                  # warm-up of both arms at this shape
        timed(arm_b)
        ta, tb = [], []
        for _ in range(a.repeats):                    # interleaved
            ta.append(timed(arm_a))
            tb.append(timed(arm_b))
        fit = last['a'].check()
        ja, jb = fit.objective()[-1].item(), last['b'][1].item()
        nbytes, flops = algorithmic(n, nc, N, T)
        A, B = summary(ta), summary(tb)
        out = {'n_fine': n, 'nc': nc, 'N': N, 'kernel': A, 'module_loop': B,
               'speedup': B['median_ms'] / A['median_ms'],
               'final_objective': {'kernel': ja, 'module_loop': jb},
               'kernel_bytes': nbytes, 'kernel_GBps': nbytes / (A['median_ms'] * 1e-3) / 1e9,
               'flops_per_iteration_per_sample': flops,
               'kernel_GFLOPs': flops * T * N / (A['median_ms'] * 1e-3) / 1e9,
               'us_per_iteration': A['median_ms'] * 1e3 / T}
        res['shapes']['%dx%d_N%d' % (n, n, N)] = out
        print('%3d x %3d nc %d N %4d | kernel %.2f ms (%.2f..%.2f) | module loop %.2f ms (%.2f..%.2f) | x %.1f | '
              '%.1f us / iteration, %.2f GB/s, %.1f GFLOP/s | J %.4e / %.4e'
              % (n, n, nc, N, A['median_ms'], A['min_ms'], A['max_ms'], B['median_ms'], B['min_ms'], B['max_ms'],
                 out['speedup'], out['us_per_iteration'], out['kernel_GBps'], out['kernel_GFLOPs'], ja, jb), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
        fh.write('\n')
    print('wrote', a.out)


if __name__ == '__main__':
    main()
