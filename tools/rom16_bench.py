"""Cost of the 16 x 16 coarse-grained model: gpi_rom at nc = 16 by its native kernels and by the generic
barrier-per-step kernel, and what the finer coarse mesh costs a whole training step.

GPI_ROM_SLOW is read once per process, so the two kernel arms run as fresh child processes, started alternately
and one after another by a parent that never touches the GPU (`--alternations` pairs, >= 5).  Each child warms
up, captures 200 launches into one HIP graph and times replays of it with HIP events; reported per arm: the
median (min..max) over the children of each child's median replay, in us per launch.
  (a) LOGLIK (solve + W u + log-likelihood + adjoint), N = 32, r = 8 (128 x 128) and r = 16 (256 x 256)
  (b) the coarse-only forward (FORWARD with uc, no mu_y: the VO MC predictive's solves), N = 16 384
  (c) one more child, arms interleaved inside it: the captured fused step at 128 x 128, B_u = 256 + N_s = 32, for
      highres128 (8 x 8 coarse mesh) and highres128_rom16, ms per step.  At d_x = 512 the head runs its VALU
      kernels (the MFMA head holds rows of at most 256), so (c) carries that cost too.

    python tools/rom16_bench.py --out profiles/rom16_bench.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'generative-physics-informed-pde_amd'))

NC = 16
LAUNCHES = 200
CASES = [('loglik_r8_N32', 'loglik', 8, 32), ('loglik_r16_N32', 'loglik', 16, 32), ('coarse_N16384', 'coarse', 8, 16384)]


def summary(xs, unit):
    return {'median_' + unit: statistics.median(xs), 'min_' + unit: min(xs), 'max_' + unit: max(xs), 'repeats': len(xs)}


def child_rom(replays):
    """us per launch of every case in this process's arm -> one JSON line."""
    import numpy as np
    import torch
    from gpi import _lib as L
    from gpi.engine import rom_call
    dev = torch.device('cuda:0')
    out = {}
    for name, kind, r, N in CASES:
        rng = np.random.default_rng(N + r)
        n = NC * r
        dy, nn = (n + 1) * (n - 1), (NC + 1) ** 2
        t = lambda a: torch.tensor(a, dtype=torch.float32, device=dev)
        x = t(rng.normal(0.3, 0.7, (N, 2 * NC * NC)))
        F = np.zeros((N, nn), dtype=np.float32)
        bn = [e for e in range(nn) if e % (NC + 1) in (0, NC)]
        F[:, bn] = rng.uniform(-0.5, 0.5, (N, len(bn)))
        F = t(F)
        uc = torch.empty(N, nn, device=dev)
        if kind == 'loglik':
            mu = torch.empty(N, dy, device=dev)
            rom_call(NC, r, x, F, False, L.ROM_FORWARD, mu_y=mu)
            Y = mu + 0.3 * torch.randn(mu.shape, device=dev, generator=torch.Generator(dev).manual_seed(N))
            ls = t(np.log(0.3) + 0.1 * rng.normal(size=dy))
            gx = torch.zeros_like(x)
            part = torch.empty(N, dy, device=dev)
            acc = torch.zeros(L.GPI_REPLICAS, dtype=torch.float64, device=dev)
            flag = torch.zeros(1, dtype=torch.int32, device=dev)
            launch = lambda: rom_call(NC, r, x, F, False, L.ROM_LOGLIK, Y=Y, logsig_y=ls, gx=gx, gls_part=part,
                                      loss_acc=acc, flag=flag)
        else:
            launch = lambda: rom_call(NC, r, x, F, False, L.ROM_FORWARD, uc=uc)
        many = LAUNCHES
        nrep = replays if kind == 'loglik' else min(replays, 3)   # the generic coarse-only arm takes ms per launch
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            for _ in range(3):
                launch()
            s.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                for _ in range(many):
                    launch()
            g.replay()
            s.synchronize()
            ts = []
            for _ in range(nrep):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
                g.replay()
                e1.record(s)
                e1.synchronize()
                ts.append(1e3 * e0.elapsed_time(e1) / many)
        out[name] = statistics.median(ts)
    print('RESULT ' + json.dumps(out), flush=True)


def child_step(replays, steps):
    """ms per captured fused step at 128 x 128, bench.py's c128 batch, 8 x 8 vs 16 x 16 coarse mesh, interleaved."""
    import torch
    import bench
    from gpi.train import FusedElboStep
    bench.CONFIGS['c128_rom16'] = ('highres128_rom16',) + bench.CONFIGS['c128'][1:]
    dev = torch.device('cuda:0')
    arms = {}
    for cfg in ('c128', 'c128_rom16'):
        model, (Xu, Xs, Y, F), (B_u, N_s), _ = bench.build(cfg, dev, seed=1000)
        step = FusedElboStep(model, Xu, B_u, Xs, Y, F, lr=1e-2, seed=4321, subset_seed=777)
        step.capture()
        step.run(5)
        torch.cuda.synchronize()
        arms[cfg] = step
    ts = {k: [] for k in arms}
    for _ in range(replays):
        for k, step in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            step.run(steps)
            e1.record()
            e1.synchronize()
            ts[k].append(e0.elapsed_time(e1) / steps)
    for step in arms.values():
        step.engine.check_flag()
    print('RESULT ' + json.dumps({k: summary(v, 'ms') for k, v in ts.items()}), flush=True)


def run_child(args, env):
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, env=env, capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit('child %s failed (%d):\n%s\n%s' % (args, r.returncode, r.stdout[-2000:], r.stderr[-4000:]))
    line = [l for l in r.stdout.splitlines() if l.startswith('RESULT ')][-1]
    return json.loads(line[7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--alternations', type=int, default=5)
    ap.add_argument('--replays', type=int, default=7)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--child', choices=['rom', 'step'])
    ap.add_argument('--skip-step', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'rom16_bench.json'))
    a = ap.parse_args()
    if a.child == 'rom':
        return child_rom(a.replays)
    if a.child == 'step':
        return child_step(a.replays, a.steps)
    base = {k: v for k, v in os.environ.items() if k != 'GPI_ROM_SLOW'}
    runs = {'native': [], 'generic': []}
    for i in range(max(a.alternations, 5)):
        for arm in ('native', 'generic'):
            env = dict(base, GPI_ROM_SLOW='1') if arm == 'generic' else base
            runs[arm].append(run_child(['--child', 'rom', '--replays', str(a.replays)], env))
            print(i, arm, runs[arm][-1], flush=True)
    res = {'launches_per_graph': LAUNCHES, 'alternations': len(runs['native']), 'nc': NC,
           'rom': {}}
    for name, _, r, N in CASES:
        nat = summary([c[name] for c in runs['native']], 'us')
        gen = summary([c[name] for c in runs['generic']], 'us')
        res['rom'][name] = {'refine': r, 'N': N, 'native': nat, 'generic': gen,
                            'speedup': gen['median_us'] / nat['median_us']}
        print('%-16s native %.1f us (%.1f..%.1f) | generic %.1f us (%.1f..%.1f) | x %.1f'
              % (name, nat['median_us'], nat['min_us'], nat['max_us'], gen['median_us'], gen['min_us'], gen['max_us'],
                 res['rom'][name]['speedup']), flush=True)
    if not a.skip_step:
        st = run_child(['--child', 'step', '--replays', str(a.replays), '--steps', str(a.steps)], base)
        res['fused_step_128'] = {'B_u': 256, 'N_s': 32, 'highres128': st['c128'], 'highres128_rom16': st['c128_rom16']}
        print('fused step 128 x 128: 8 x 8 mesh %.3f ms (%.3f..%.3f) | 16 x 16 mesh %.3f ms (%.3f..%.3f)'
              % (st['c128']['median_ms'], st['c128']['min_ms'], st['c128']['max_ms'], st['c128_rom16']['median_ms'],
                 st['c128_rom16']['min_ms'], st['c128_rom16']['max_ms']), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
        fh.write('\n')
    print('wrote', a.out)


if __name__ == '__main__':
    main()
