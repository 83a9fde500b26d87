"""Cost of hidden layers in the effective-property map (gp as an MLP, csrc/gpmlp.hip) in the captured fused step.

Arms, all in this one process, interleaved round-robin over the repeats:
    c64   the 64^2 bench step (bench.py c64: highres, B_u = 256, N_s = 32) with L = 0, 1, 2 hidden layers
          (64 -> 128; 64 -> 96 -> 128; 64 -> 85 -> 106 -> 128)
    c128  the same batch at 128^2 on highres128_rom16 with L = 0, 1 (64 -> 512; 64 -> 288 -> 512)
Method: HIP events around `steps` graph replays after a warm-up, median and min / max of `repeats` timings per arm;
the L >= 1 arms are reported against the L = 0 arm of the same run.  The two launches' own algorithmic work is
listed per arm (flops = 2 x rows x sum of layer products, forward; twice that backward without the weight GEMMs;
bytes = the weights once per workgroup of 16 rows plus the rows' activations) -- their device times come from a
separate kernel-trace run of this script with --arms and --repeats 1.

--parent DIR (a checkout of the parent commit with its library built) adds the guard of the unchanged default path:
the c64 L = 0 step of this checkout beside the parent's, one fresh child process per arm and repeat (two checkouts
cannot share a process), alternated; this checkout's median must lie inside the parent's min-max spread.

usage: python tools/gpmlp_bench.py [out.json] [--steps K] [--repeats R] [--arms c64:0,c64:1,...] [--parent DIR]
"""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _paths(root):
    for p in (root, os.path.join(root, 'generative-physics-informed-pde_amd')):
        if p not in sys.path:
            sys.path.insert(0, p)

ARMS = ['c64:0', 'c64:1', 'c64:2', 'c128:0', 'c128:1']
FACTORY = {'c64': None, 'c128': 'highres128_rom16'}        # None: the bench configuration's own factory


def build_step(cfg, L, seed=4321):
    import torch
    import bench
    from factories.model import ModelFactory
    from gpi.train import FusedElboStep
    real = ModelFactory.FromIdentifier
    swap = FACTORY[cfg]
    ModelFactory.FromIdentifier = classmethod(
        lambda cls, ident, *a, **k: real(swap or ident, *a, eff_property_map_hidden_layers=L, **k))
    try:
        model, (Xu, Xs, Y, F), (B_u, N_s), _ = bench.build(cfg, torch.device('cuda', 0), 1234)
    finally:
        ModelFactory.FromIdentifier = real
    step = FusedElboStep(model, Xu, B_u, Xs, Y, F, lr=1e-4, seed=seed)
    step.capture()
    return step


def timed(fn, k):
    import torch
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    for _ in range(k):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / k


def work(e):
    """Algorithmic flops / bytes of the step's two MLP launches."""
    w, n = e.gp_widths, e.N_x
    if not w:
        return None
    prod = sum(a * b for a, b in zip(w[:-1], w[1:]))
    tiles = (n + 15) // 16
    act = n * (sum(w) + 3 * w[-1])
    return dict(widths=w, rows=n, forward_flops=2 * n * prod, backward_flops=2 * n * prod,
                forward_bytes=4 * (tiles * (prod + sum(w[1:])) + act),
                backward_bytes=4 * (tiles * prod + 2 * act))


def worker(steps):
    """One timing of the default (L = 0) c64 step in this fresh process, from the checkout on sys.path."""
    import torch
    import bench
    from gpi.train import FusedElboStep
    model, (Xu, Xs, Y, F), (B_u, N_s), _ = bench.build('c64', torch.device('cuda', 0), 1234)
    step = FusedElboStep(model, Xu, B_u, Xs, Y, F, lr=1e-4, seed=4321)
    step.capture()
    timed(step.step, max(steps // 2, 20))
    ms = timed(step.step, steps)
    step.check_handoff()
    print(json.dumps(dict(ms=ms, finite=bool(torch.isfinite(step.elbo()).item()))))


def guard(parent, steps, repeats):
    import subprocess
    ms = {'parent': [], 'this': []}
    for _ in range(repeats):
        for name, root in (('parent', parent), ('this', ROOT)):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), '--worker', '--root', root, '--steps',
                                  str(steps)], check=True, capture_output=True, text=True, timeout=300).stdout
            r = json.loads(out.strip().splitlines()[-1])
            assert r['finite']
            ms[name].append(r['ms'])
    res = {k: stats(v) for k, v in ms.items()}
    res['inside_parent_spread'] = bool(res['parent']['min'] <= res['this']['median'] <= res['parent']['max'])
    return res


def stats(v):
    return dict(median=round(statistics.median(v), 5), min=round(min(v), 5), max=round(max(v), 5))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('out', nargs='?', default=os.path.join(ROOT, 'profiles', 'gpmlp_bench.json'))
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--repeats', type=int, default=9)
    ap.add_argument('--arms', default=','.join(ARMS))
    ap.add_argument('--parent', default=None)
    ap.add_argument('--worker', action='store_true')
    ap.add_argument('--root', default=ROOT)
    args = ap.parse_args()
    _paths(args.root)
    if args.worker:
        return worker(args.steps)
    import torch
    arms = args.arms.split(',')
    steps = {}
    for a in arms:
        cfg, L = a.split(':')
        steps[a] = build_step(cfg, int(L))
        assert steps[a].engine.gp_hidden == int(L)
        timed(steps[a].step, max(args.steps // 2, 20))
    ms = {a: [] for a in arms}
    for _ in range(args.repeats):
        for a in arms:
            ms[a].append(timed(steps[a].step, args.steps))
    res = dict(device=torch.cuda.get_device_name(0), steps=args.steps, repeats=args.repeats,
               method='HIP events around graph replays, arms interleaved per repeat, median and min / max of the '
                      'repeats; ms per step', arms={})
    for a in arms:
        s = steps[a]
        s.check_handoff()
        s.engine.check_flag()
        r = dict(ms=stats(ms[a]), finite=bool(torch.isfinite(s.elbo()).item()), mlp=work(s.engine))
        base = a.split(':')[0] + ':0'
        if base in ms and base != a:
            r['over_L0_ms'] = round(statistics.median(ms[a]) - statistics.median(ms[base]), 5)
        res['arms'][a] = r
        print(a, r)
    if args.parent:
        del steps
        torch.cuda.empty_cache()
        res['default_step_vs_parent'] = guard(os.path.abspath(args.parent), args.steps, args.repeats)
        print('default step vs parent', res['default_step_vs_parent'])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(res, fh, indent=1)


if __name__ == '__main__':
    main()
