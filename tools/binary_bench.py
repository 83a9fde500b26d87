"""The binary (two-phase) decoder path, timed at the bench codec (bench.py c64: 64^2, B_u = 256, N_s = 32, decoder
batch 288):

  (a) launch   the fused output conv alone (gpi_conv_loss_fused on the captured step's own descriptor and
               context, K launches per graph replay): the Bernoulli one-channel instantiation against the Gaussian
               one, both on the generic kernels (GPI_CONV_SHAPES=0 for the Gaussian arm; the Bernoulli launch has
               no compile-time shape entry);
  (b) step     the captured fused step of `highres` with binary_field=True (two-valued fields) beside the Gaussian
               step of the parent checkout (--parent DIR: a checkout of the parent commit with its library built);
  (c) guard    the Gaussian step of this checkout beside the parent's (the conv kernels' by-value context grew by
               tgt_lo: every kernel touches the whole argument block at entry).

Method (as tools/vo_step_bench.py): HIP events around graph replays after a warm-up, the arms interleaved round-robin
over the repeats, median and spread (min / max) of the repeats.  (a) runs in this process; each timing of (b) / (c)
is one fresh child process per arm and repeat (two checkouts cannot share a process), so their spread includes
process-to-process variation.

usage: python tools/binary_bench.py [out.json] [--parent DIR] [--steps K] [--repeats R]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _paths(root):
    for p in (root, os.path.join(root, 'generative-physics-informed-pde_amd')):
        if p not in sys.path:
            sys.path.insert(0, p)


def build_step(binary, seed=4321):
    """The captured bench step (c64) and its model; binary: the factory's binary_field=True and the fields
    thresholded at their medians into log 1 / log 10."""
    import torch
    import bench
    from factories.model import ModelFactory
    from gpi.train import FusedElboStep
    dev = torch.device('cuda', 0)
    real = ModelFactory.FromIdentifier
    if binary:
        ModelFactory.FromIdentifier = classmethod(lambda cls, ident, *a, **k: real(ident, *a, binary_field=True, **k))
    try:
        model, (Xu, Xs, Y, F), (B_u, N_s), _ = bench.build('c64', dev, 1234)
    finally:
        if binary:
            ModelFactory.FromIdentifier = real
    if binary:
        import math

        def two_phase(X):
            med = X.flatten(1).median(1).values[:, None, None]
            return torch.where(X > med, math.log(10.0), math.log(1.0)).to(X.dtype).contiguous()

        Xu, Xs = two_phase(Xu), two_phase(Xs)
        model._datasets['unsupervised'].t['X'] = Xu
        model._datasets['supervised'].t['X'] = Xs
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


def worker(arm, steps):
    """One timing of a step arm in this (fresh) process: ms per step."""
    import torch
    step = build_step(arm == 'binary_step')
    timed(step.step, max(steps // 2, 20))
    ms = timed(step.step, steps)
    step.check_handoff()
    step.engine.check_flag()
    print(json.dumps(dict(ms=ms, finite=bool(torch.isfinite(step.elbo()).item()))))


def launch_graph(step, k, shapes_off):
    """A graph of k gpi_conv_loss_fused launches of the step's output conv (its descriptor, its context; the
    operands are what the step's last forward left)."""
    import ctypes as C
    import torch
    from gpi import _lib as L
    e = step.engine
    d = e.dec_descs[len(e.dec_descs) - 1]
    lib = L.lib()
    old = os.environ.get('GPI_CONV_SHAPES')
    if shapes_off:
        os.environ['GPI_CONV_SHAPES'] = '0'
    try:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(k):
                L.check(lib.gpi_conv_loss_fused(C.byref(d), C.byref(e.dctx), L.stream_handle()), 'fused output conv')
    finally:
        if shapes_off:
            if old is None:
                del os.environ['GPI_CONV_SHAPES']
            else:
                os.environ['GPI_CONV_SHAPES'] = old
    return g, dict(cin=d.cin, cout=d.cout, plane=(d.h_out, d.w_out), batch=e.B, epilogue=d.epilogue)


def stats(v):
    return dict(median=round(statistics.median(v), 5), min=round(min(v), 5), max=round(max(v), 5))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('out', nargs='?')
    ap.add_argument('--parent', default=None, help='checkout of the parent commit (library built) for (b) / (c)')
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--repeats', type=int, default=9)
    ap.add_argument('--launches', type=int, default=50, help='(a): launches per graph replay')
    ap.add_argument('--worker', default=None, choices=['gauss_step', 'binary_step'])
    ap.add_argument('--root', default=ROOT)
    args = ap.parse_args()
    _paths(args.root)
    if args.worker:
        return worker(args.worker, args.steps)
    import torch
    res = dict(config='c64 (64^2, B_u = 256, N_s = 32: decoder batch 288)', device=torch.cuda.get_device_name(0),
               repeats=args.repeats, method='HIP events around graph replays, arms interleaved per repeat, median '
               'and min / max of the repeats')
    # ---- (a) the launch
    sg, sb = build_step(False), build_step(True)
    for s in (sg, sb):
        timed(s.step, 20)
    graphs = {}
    graphs['gauss_generic'], dg = launch_graph(sg, args.launches, True)
    graphs['bernoulli'], db = launch_graph(sb, args.launches, False)
    for g in graphs.values():
        timed(g.replay, 5)
    us = {k: [] for k in graphs}
    for _ in range(args.repeats):
        for k, g in graphs.items():
            us[k].append(timed(g.replay, 4) / args.launches * 1e3)
    a = {k: stats(v) for k, v in us.items()}
    spread = a['gauss_generic']['max'] - a['gauss_generic']['min']
    res['a_launch_us'] = dict(a, ops=dict(gauss_generic=dg, bernoulli=db), launches_per_replay=args.launches,
                              gauss_spread=round(spread, 5),
                              bernoulli_no_slower_than_gauss_plus_spread=bool(
                                  a['bernoulli']['median'] <= a['gauss_generic']['median'] + spread))
    del graphs, sg, sb
    torch.cuda.empty_cache()
    # ---- (b), (c) the steps, one child process per timing
    arms = [('gauss_step_head', 'gauss_step', ROOT), ('binary_step_head', 'binary_step', ROOT)]
    if args.parent:
        arms.insert(0, ('gauss_step_parent', 'gauss_step', os.path.abspath(args.parent)))
    ms = {name: [] for name, _, _ in arms}
    for _ in range(args.repeats):
        for name, arm, root in arms:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), '--worker', arm, '--root', root, '--steps',
                                  str(args.steps)], check=True, capture_output=True, text=True, cwd=root,
                                 timeout=300).stdout
            r = json.loads(out.strip().splitlines()[-1])
            assert r['finite'], name
            ms[name].append(r['ms'])
    res['bc_step_ms'] = dict({k: stats(v) for k, v in ms.items()}, steps_per_timing=args.steps,
                             note='one fresh process per arm and repeat; binary_step_head runs its output conv on '
                             'the generic kernel (no compile-time shape entry for the Bernoulli launch)')
    if args.parent:
        p, h = res['bc_step_ms']['gauss_step_parent'], res['bc_step_ms']['gauss_step_head']
        res['c_gauss_head_within_parent_spread'] = bool(h['median'] <= p['median'] + (p['max'] - p['min']))
    print(json.dumps(res))
    if args.out:
        with open(args.out, 'w') as fh:
            json.dump(res, fh, indent=1)


if __name__ == '__main__':
    main()
