"""FusedElboStep(l2_penalty=), timed at the bench codec (bench.py c64: 64^2, B_u = 256, N_s = 32):

  (1) guard    the default step (l2_penalty=None) of this checkout beside the parent's (--parent DIR: a checkout of
               the parent commit with its library built), alternating fresh processes (the epilogue kernels'
               by-value descriptor grew by the penalty's four fields), and the arrays bench.py --dump-outputs leaves
               compared bit for bit;
  (2) step     the captured step with a penalty beside the captured step without one, both in this process, the arms
               interleaved per repeat;
  (3) launch   gpi_param_norms alone (K launches per graph replay) on the c64 model's flat buffer and on highres256
               with homoscedastic=True, whose noise plane is one segment of 65 536 floats.

Method (as tools/homosc_bench.py): HIP events around graph replays after a warm-up, median and spread (min / max) of
the repeats, one box.  Each timing of (1) is one fresh child process per arm and repeat (two checkouts cannot share a
process), so its spread includes process-to-process variation.

usage: python tools/l2_bench.py [out.json] [--parent DIR] [--steps K] [--repeats R]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
from homosc_bench import _paths, timed, stats, dump_equal  # noqa: E402

L2 = 0.05           # the reference fixtures' factor (the cost does not depend on the value)


def build_step(l2, seed=4321):
    """The captured bench step (c64); l2 None: built without the keyword (the parent's constructor has none)."""
    import torch
    import bench
    from gpi.train import FusedElboStep
    model, (Xu, Xs, Y, F), (B_u, N_s), _ = bench.build('c64', torch.device('cuda', 0), 1234)
    kw = {} if l2 is None else dict(l2_penalty=l2)
    step = FusedElboStep(model, Xu, B_u, Xs, Y, F, lr=1e-4, seed=seed, **kw)
    step.capture()
    return step


def worker(steps):
    """One timing of the default step in this (fresh) process: ms per step."""
    import torch
    step = build_step(None)
    timed(step.step, max(steps // 2, 20))
    ms = timed(step.step, steps)
    step.check_handoff()
    step.engine.check_flag()
    print(json.dumps(dict(ms=ms, finite=bool(torch.isfinite(step.elbo()).item()))))


def norms_graph(model, k):
    """A graph of k gpi_param_norms launches over the model's penalised tensors; the buffers it needs."""
    import torch
    from gpi import _lib as L
    from gpi.train import l2_segments
    flat = model.native_flat()
    rows = l2_segments(model, flat)
    table = [v for _, o, n in rows for v in (o, n)]
    pen_n = max(o + n for _, o, n in rows)
    dev = flat.P.device
    keep = dict(host=(C.c_int64 * len(table))(*table), seg=torch.tensor(table, dtype=torch.int64, device=dev),
                lam=torch.tensor([L2], dtype=torch.float32, device=dev),
                norms=torch.zeros(len(rows), dtype=torch.float64, device=dev),
                pen=torch.zeros(2, dtype=torch.float64, device=dev),
                grad=torch.zeros(pen_n, dtype=torch.float32, device=dev),
                done=torch.zeros(1, dtype=torch.int32, device=dev))
    d = L.ParamNormsDesc(p=flat.P.data_ptr(), seg=keep['seg'].data_ptr(), seg_host=C.addressof(keep['host']),
                         n_seg=len(rows), pen_n=pen_n, lam=keep['lam'].data_ptr(), norms=keep['norms'].data_ptr(),
                         pen=keep['pen'].data_ptr(), pen_grad=keep['grad'].data_ptr(), done=keep['done'].data_ptr())
    keep['desc'] = d
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(k):
            L.check(L.lib().gpi_param_norms(C.byref(d), L.stream_handle()), 'parameter norms')
    sizes = sorted(n for _, _, n in rows)
    return g, keep, dict(segments=len(rows), floats=sum(sizes), largest=sizes[-1], smallest=sizes[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('out', nargs='?')
    ap.add_argument('--parent', default=None, help='checkout of the parent commit (library built) for (1)')
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--repeats', type=int, default=9)
    ap.add_argument('--launches', type=int, default=50, help='(3): launches per graph replay')
    ap.add_argument('--worker', action='store_true')
    ap.add_argument('--root', default=ROOT)
    args = ap.parse_args()
    _paths(args.root)
    if args.worker:
        return worker(args.steps)
    import torch
    from factories.model import ModelFactory
    res = dict(config='c64 (64^2, B_u = 256, N_s = 32)', device=torch.cuda.get_device_name(0), repeats=args.repeats,
               l2_penalty=L2, method='HIP events around graph replays, arms interleaved per repeat, median and '
               'min / max of the repeats')
    # ---- (2) the step with and without the penalty, one process
    steps = {'step_none': build_step(None), 'step_l2': build_step(L2)}
    for s in steps.values():
        timed(s.step, max(args.steps // 2, 20))
    ms = {k: [] for k in steps}
    for _ in range(args.repeats):
        for k, s in steps.items():
            ms[k].append(timed(s.step, args.steps))
    for s in steps.values():
        s.check_handoff()
    res['step_ms'] = dict({k: stats(v) for k, v in ms.items()}, steps_per_timing=args.steps,
                          graph_mode={k: s.graph_mode for k, s in steps.items()})
    res['step_increase_us'] = round((res['step_ms']['step_l2']['median'] - res['step_ms']['step_none']['median']) * 1e3, 3)
    # ---- (3) the launch alone
    graphs = {}
    graphs['c64'] = norms_graph(steps['step_l2'].model, args.launches)
    fac = ModelFactory.FromIdentifier('highres256', homoscedastic=True)
    fac.set('device', 'cuda')
    _, big, _, encoder, _, _ = fac.setup()
    big.encoder = encoder.cuda()
    big.cuda()
    graphs['highres256_homoscedastic'] = norms_graph(big, args.launches)
    for g, _, _ in graphs.values():
        timed(g.replay, 5)
    us = {k: [] for k in graphs}
    for _ in range(args.repeats):
        for k, (g, _, _) in graphs.items():
            us[k].append(timed(g.replay, 4) / args.launches * 1e3)
    res['launch_us'] = dict({k: dict(stats(v), layout=graphs[k][2]) for k, v in us.items()},
                            launches_per_replay=args.launches,
                            note='back-to-back launches on one stream: the launch boundary is part of the figure')
    del graphs, steps
    torch.cuda.empty_cache()
    # ---- (1) the default step against the parent's, one child process per timing
    if args.parent:
        arms = [('default_parent', os.path.abspath(args.parent)), ('default_head', ROOT)]
        ms = {name: [] for name, _ in arms}
        for _ in range(args.repeats):
            for name, root in arms:
                # (this file runs in both checkouts: --root says whose code)
                out = subprocess.run([sys.executable, os.path.abspath(__file__), '--worker', '--root', root, '--steps',
                                      str(args.steps)], check=True, capture_output=True, text=True, cwd=root,
                                     timeout=300).stdout
                r = json.loads(out.strip().splitlines()[-1])
                assert r['finite'], name
                ms[name].append(r['ms'])
                print('%s %.5f ms' % (name, r['ms']), file=sys.stderr, flush=True)
        g = dict({k: stats(v) for k, v in ms.items()}, steps_per_timing=args.steps,
                 note='one fresh process per arm and repeat')
        p, h = g['default_parent'], g['default_head']
        g['head_median_within_parent_min_max'] = bool(p['min'] <= h['median'] <= p['max'])
        g['head_no_slower_than_parent_max'] = bool(h['median'] <= p['max'])
        g['dump_outputs_equal_parent'] = dump_equal(os.path.abspath(args.parent))
        res['default_guard_ms'] = g
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            json.dump(res, fh, indent=1)


if __name__ == '__main__':
    main()
