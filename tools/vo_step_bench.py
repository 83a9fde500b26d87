"""The fused training step with the virtual-observable term, timed at the bench codec (bench.py c64: 64^2,
B_u = 256, N_s = 32) with N_vo = 32 VO samples (CGR + flux rows):

  fused            the captured step without VO (what bench.py times)
  fused_vo_held    X_vo given, vo_holdoff=True  (third decoder BN group, larger head; no second ROM)
  fused_vo         X_vo given, the term active  (+ second ROM launch, y_vo draw)
  module_vo        model.elbo + backward + torch Adam for the same shapes: what a VO user ran before
  vo_update        one step.update_virtual_observables(128)

Method: HIP events around K graph replays (host timer + device sync for the host-bound module loop and the
update), a warm-up, the arms interleaved round-robin over the repeats in one process, median and spread
(min / max) over the repeats.  gpi_conv_shape_info beside each arm: the decoder batch B_u + N_s + N_vo is
not in csrc/conv_shapes.h, so the VO arms' decoder launches take the generic kernels.

usage: python tools/vo_step_bench.py [out.json] [--steps K] [--repeats R]
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
import numpy as np  # noqa: E402
import torch  # noqa: E402

N_VO, N_MC = 32, 128


class _DS(object):
    def __init__(self, **t):
        self.t = t
        self.N = next(iter(t.values())).shape[0]

    def __bool__(self):
        return True

    def get(self, k, random_subset=None):
        return self.t[k] if random_subset is None else self.t[k][:random_subset]


def add_vo(model, data, physics, dev):
    """N_VO synthetic VO samples (fields / BCs as tools/vo_bench.py) registered beside the bench datasets."""
    from bottleneck import VirtualObservables as VO
    from physics.BoundaryConditions import BoundaryCondition
    from physics.grid import pixel_to_cells
    Xu, Xs, Y, F = data
    n = physics['fom'].grid.n
    rng = np.random.default_rng(3)
    X = rng.normal(0.4, 0.8, (N_VO, n, n))
    U = rng.uniform(-0.5, 0.5, (N_VO, 4))
    Fv = np.stack([physics['rom'].grid.full_force(u) for u in U])
    QPE = VO.QuerryPointEnsemble([VO.QuerryPoint(physics['fom'], pixel_to_cells(x), BoundaryCondition(u))
                                  for x, u in zip(X, U)])
    QE = VO.QuerryEnsemble.FromQuerryPointEnsemble(QPE, physics, True, True, 0, 0, dtype=torch.float32, device=dev)
    ens = VO.VirtualObservablesEnsemble(QPE, QE, dtype=torch.float32, device=dev)
    t = lambda a: torch.tensor(a, dtype=torch.float32, device=dev).contiguous()
    vo_ds = _DS(X=t(X), Y=t(np.zeros((N_VO, (n + 1) * (n - 1)))), F_ROM_BC=t(Fv))
    model.register_datasets({'supervised': _DS(X=Xs, Y=Y, F_ROM_BC=F), 'unsupervised': _DS(X=Xu), 'vo': vo_ds}, ens,
                            create_unsupervised_variational_approximation=False)
    return vo_ds, ens


def shape_info():
    import bench
    return bench.conv_shape_info()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('out', nargs='?')
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--module-steps', type=int, default=10)
    args = ap.parse_args()
    import bench
    from gpi.train import FusedElboStep
    dev = torch.device('cuda', 0)
    lr = 1e-4
    model0, (Xu, Xs, Y, F), (B_u, N_s), _ = bench.build('c64', dev, 1234)
    model1, data1, _, physics = bench.build('c64', dev, 1234)
    vo_ds, ens = add_vo(model1, data1, physics, dev)
    torch.manual_seed(1)
    for it in range(2):
        model1.update_virtual_observables(N_MC, step=it)
    Xv, Fv = vo_ds.get('X'), vo_ds.get('F_ROM_BC')
    arms, info = {}, {}

    def fused(name, model, data, **kw):
        before = shape_info()
        s = FusedElboStep(model, data[0], B_u, data[1], data[2], data[3], lr=lr, seed=4321, **kw)
        s.capture()
        after = shape_info()
        info[name] = dict(graph_mode=s.graph_mode, decoder_batch=s.engine.B, conv_shape_table=after['table'],
                          conv_launches_planned=after['launches_planned'] - before['launches_planned'],
                          conv_launches_on_shape=after['on_shape'] - before['on_shape'])
        arms[name] = s
        return s

    fused('fused', model0, (Xu, Xs, Y, F))
    fused('fused_vo_held', model1, data1, X_vo=Xv, F_vo=Fv, vo_holdoff=True)
    step_vo = fused('fused_vo', model1, data1, X_vo=Xv, F_vo=Fv)
    opt = torch.optim.Adam(model1.parameters(), lr=lr)

    def module_step():
        opt.zero_grad()
        elbo = model1.elbo(step=0, armortized_bs=B_u)
        (-elbo).backward()
        opt.step()

    def timed(fn, k):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        w0 = time.perf_counter()
        t0.record()
        for _ in range(k):
            fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) / k, (time.perf_counter() - w0) * 1e3 / k

    runs = {name: (s.step, args.steps) for name, s in arms.items()}
    runs['module_vo'] = (module_step, args.module_steps)
    before = shape_info()
    for name, (fn, k) in runs.items():          # warm-up (module path: engine build, allocator)
        timed(fn, max(k // 4, 3))
    after = shape_info()
    info['module_vo'] = dict(decoder_batch=B_u + N_s + N_VO, note='launches planned by every step (no graph)',
                             conv_launches_planned_warmup=after['launches_planned'] - before['launches_planned'],
                             conv_launches_on_shape_warmup=after['on_shape'] - before['on_shape'])
    ms = {name: [] for name in runs}
    wall = {name: [] for name in runs}
    upd = []
    for r in range(args.repeats):               # interleaved: every repeat visits every arm in the same order
        for name, (fn, k) in runs.items():
            dev_ms, wall_ms = timed(fn, k)
            ms[name].append(dev_ms)
            wall[name].append(wall_ms)
        torch.cuda.synchronize()
        w0 = time.perf_counter()
        step_vo.update_virtual_observables(N_MC, step=2 + r)
        upd.append((time.perf_counter() - w0) * 1e3)
    for s in arms.values():
        s.check_handoff()
        s.engine.check_flag()
    ens.check_flag()

    def stats(v):
        return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))

    res = dict(config='c64 (64^2, B_u = %d, N_s = %d), N_vo = %d, CGR + flux rows' % (B_u, N_s, N_VO),
               device=torch.cuda.get_device_name(0), steps_per_timing=args.steps, repeats=args.repeats,
               method='HIP events around K graph replays, arms interleaved per repeat, one process; ms per step',
               ms_per_step={k: stats(v) for k, v in ms.items()},
               wall_ms_per_step={k: stats(v) for k, v in wall.items()},
               vo_update_ms=dict(N_mc=N_MC, host_timer_with_device_sync=True, **stats(upd)),
               conv_shape_info=info, elbo_finite={k: bool(torch.isfinite(s.elbo()).item()) for k, s in arms.items()})
    print(json.dumps(res))
    if args.out:
        with open(args.out, 'w') as fh:
            json.dump(res, fh, indent=1)


if __name__ == '__main__':
    main()
