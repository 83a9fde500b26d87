"""Bit digests of gpi_rom / gpi_rom_fit outputs, to compare two builds of csrc/rom.hip.

Seeded inputs at the smallest shapes that reach every kernel and mode of rom.hip; one sha256 per output buffer.
The library and GPI_ROM_SLOW / GPI_ROM_FAST_NT are read once per process, so the driver runs every arm as a
fresh child (`--arm`), one after another, each under its own timeout, and stops at the first failure:
  parent, parent2   GPI_LIB_VARIANT=parent GPI_ALLOW_STALE_LIB=1 (libgpi_hip_parent.so, built from the parent's
                    csrc: make -C csrc OUT=../gpi/libgpi_hip_parent.so BUILD=build_parent), twice
  new               the library of this tree
each once more with GPI_ROM_SLOW=1 (nc = 8, 16) and GPI_ROM_FAST_NT=256 / 1024 (nc = 8).  A buffer whose digest
agrees between the two parent arms must have that digest in the new arm; the others are listed.

    python tools/rom_digest.py > profiles/rom_refactor_digest.txt
"""
import argparse
import ctypes as C
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'generative-physics-informed-pde_amd'))

# environment arm -> the nc values it runs
ENVS = [('default', {}, (3, 4, 8, 16)), ('slow', {'GPI_ROM_SLOW': '1'}, (8, 16)),
        ('nt256', {'GPI_ROM_FAST_NT': '256'}, (8,)), ('nt1024', {'GPI_ROM_FAST_NT': '1024'}, (8,))]


def child(ncs, fit):
    import numpy as np
    import torch
    from gpi import _lib as L
    dev = torch.device('cuda:0')
    lib, st = L.lib(), L.stream_handle()
    t = lambda a, dt=torch.float32: torch.tensor(np.ascontiguousarray(a), dtype=dt, device=dev)
    p = lambda x: x.data_ptr() if x is not None else None

    def emit(case, **bufs):
        torch.cuda.synchronize()
        for k, v in bufs.items():
            print('DIGEST %s/%s %s' % (case, k, hashlib.sha256(v.cpu().numpy().tobytes()).hexdigest()), flush=True)

    def inputs(nc, r, N, seed):
        rng = np.random.default_rng(seed)
        nf, nn, nt = nc * r, (nc + 1) ** 2, 2 * nc * nc
        dy = (nf + 1) * (nf - 1)
        F = np.zeros((N, nn), np.float32)
        bn = [e for e in range(nn) if e % (nc + 1) in (0, nc)]
        F[:, bn] = rng.uniform(-0.5, 0.5, (N, len(bn)))
        return rng, nn, nt, dy, t(rng.normal(0.2, 0.6, (N, nt))), t(F)

    def rom(nc, r, N, x, F, mode, **kw):
        d = L.RomDesc()
        d.nc, d.refine, d.n, d.mode = nc, r, N, mode
        d.x, d.x_stride, d.F = x.data_ptr(), x.stride(0), F.data_ptr()
        d.loss_scale = 1.0
        for k, v in kw.items():
            setattr(d, k, p(v) if isinstance(v, torch.Tensor) else v)
        L.check(lib.gpi_rom(C.byref(d), st), 'gpi_rom')

    for nc in ncs:
        for r in (1, 2):
            N = 3
            rng, nn, nt, dy, x, F = inputs(nc, r, N, 100 * nc + r)
            tag = 'rom nc%d r%d' % (nc, r)
            flag = torch.zeros(1, dtype=torch.int32, device=dev)
            mu, uc = torch.zeros(N, dy, device=dev), torch.zeros(N, nn, device=dev)
            rom(nc, r, N, x, F, L.ROM_FORWARD, mu_y=mu, uc=uc, flag=flag)
            emit(tag + ' forward', mu_y=mu, uc=uc)
            Nc = 65 if nc in (4, 8) else 3                   # ragged second wave / ragged workgroup
            _, _, _, _, xc, Fc = inputs(nc, r, Nc, 100 * nc + r + 50)
            ucc = torch.zeros(Nc, nn, device=dev)
            rom(nc, r, Nc, xc, Fc, L.ROM_FORWARD, uc=ucc, flag=flag)
            emit(tag + ' coarse N%d' % Nc, uc=ucc)
            Y = mu + t(0.3 * rng.standard_normal((N, dy)))
            ls = t(np.log(0.3) + 0.1 * rng.standard_normal(dy))
            gx, part = torch.zeros(N, nt, device=dev), torch.zeros(N, dy, device=dev)
            acc = torch.zeros(L.GPI_REPLICAS, dtype=torch.float64, device=dev)
            rom(nc, r, N, x, F, L.ROM_LOGLIK, Y=Y, logsig_y=ls, gx=gx, gx_stride=nt, gls_part=part, loss_acc=acc,
                uc=uc, flag=flag, loss_scale=0.5)
            emit(tag + ' loglik', gx=gx, gls_part=part, loss_acc=acc, uc=uc)
            gacc = torch.zeros(dy, dtype=torch.float64, device=dev)
            acc.zero_()
            rom(nc, r, N, x, F, L.ROM_LOGLIK, Y=Y, logsig_y=ls, gx=gx, gx_stride=nt, gacc_logsig=gacc, loss_acc=acc,
                flag=flag)
            emit(tag + ' loglik atomics', gx=gx, gacc_logsig=gacc, loss_acc=acc)
            dmu, duc = t(rng.standard_normal((N, dy))), t(rng.standard_normal((N, nn)))
            rom(nc, r, N, x, F, L.ROM_BACKWARD, dmu=dmu, duc=duc, gx=gx, gx_stride=nt, flag=flag)
            emit(tag + ' backward', gx=gx)
            # kappa given directly; x drawn in the kernel; gradients accumulated into rows of a wider buffer
            kap = torch.exp(x) + 0.1
            rom(nc, r, N, kap, F, L.ROM_BACKWARD, input_kappa=1, dmu=dmu, mu_y=mu, gx=gx, gx_stride=nt, flag=flag)
            emit(tag + ' input_kappa', gx=gx, mu_y=mu)
            xls, xeps = t(rng.normal(-1.5, 0.2, (N, nt))), t(rng.standard_normal((N, nt)))
            gxw = t(rng.standard_normal((N, nt + 5)))
            rom(nc, r, N, x, F, L.ROM_BACKWARD, x_draw=1, x_mu=x, x_ls=xls, x_eps=xeps, duc=duc, uc=uc, gx=gxw,
                gx_stride=nt + 5, gx_accumulate=1, flag=flag)
            emit(tag + ' x_draw accumulate', gx=gxw, uc=uc, flag=flag)
    for nc in (fit or ()):
        r, N, T = 2, 2, 3
        rng, nn, nt, dy, x, F = inputs(nc, r, N, 7000 + nc)
        mu = torch.zeros(N, dy, device=dev)
        rom(nc, r, N, x, F, L.ROM_FORWARD, mu_y=mu)
        Y = mu + t(0.05 * rng.standard_normal((N, dy)))
        xf = t(0.1 * rng.standard_normal((N, nt)))
        m, v = t(0.01 * rng.standard_normal((N, nt))), t(1e-4 * rng.random((N, nt)))
        xe, uc = torch.zeros(N, nt, device=dev), torch.zeros(N, nn, device=dev)
        ss = torch.zeros(T, N, dtype=torch.float64, device=dev)
        yn = torch.zeros(N, dtype=torch.float64, device=dev)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        d = L.RomFitDesc()
        d.nc, d.refine, d.n, d.iters, d.n_total, d.step0 = nc, r, N, T, N, 4
        d.Y, d.F, d.x, d.x_stride, d.m, d.v = p(Y), p(F), p(xf), nt, p(m), p(v)
        d.lr, d.beta1, d.beta2, d.eps = 1e-2, 0.9, 0.999, 1e-8
        d.sumsq, d.ynorm2, d.x_eval, d.uc, d.flag = p(ss), p(yn), p(xe), p(uc), p(flag)
        L.check(lib.gpi_rom_fit(C.byref(d), st), 'gpi_rom_fit')
        emit('fit nc%d' % nc, x=xf, m=m, v=v, x_eval=xe, uc=uc, sumsq=ss, ynorm2=yn, flag=flag)
    print('ARM OK', flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--arm', help='child: comma-separated nc values of gpi_rom')
    ap.add_argument('--fit', default='', help='child: comma-separated nc values of gpi_rom_fit')
    ap.add_argument('--timeout', type=int, default=180)
    a = ap.parse_args()
    if a.arm is not None:
        return child([int(s) for s in a.arm.split(',') if s], [int(s) for s in a.fit.split(',') if s])
    base = {k: v for k, v in os.environ.items()
            if k not in ('GPI_ROM_SLOW', 'GPI_ROM_FAST_NT', 'GPI_LIB_VARIANT', 'GPI_ALLOW_STALE_LIB')}
    got = {}
    for lib in ('parent', 'parent2', 'new'):
        for name, extra, ncs in ENVS:
            env = dict(base, **extra)
            if lib != 'new':
                env.update(GPI_LIB_VARIANT='parent', GPI_ALLOW_STALE_LIB='1')
            cmd = ['timeout', '-k', '10', str(a.timeout), sys.executable, os.path.abspath(__file__), '--arm',
                   ','.join(map(str, ncs)), '--fit', '4,8,16' if name == 'default' else '']
            r = subprocess.run(cmd, env=env, capture_output=True, text=True)
            if r.returncode != 0 or 'ARM OK' not in r.stdout:
                raise SystemExit('arm %s/%s failed (%d):\n%s\n%s' % (lib, name, r.returncode, r.stdout[-2000:], r.stderr[-4000:]))
            got[lib, name] = dict(l.split(' ', 1)[1].rsplit(' ', 1) for l in r.stdout.splitlines() if l.startswith('DIGEST '))
    differ, unstable = [], []
    for name, _, _ in ENVS:
        for buf, h in got['parent', name].items():
            stable = got['parent2', name][buf] == h
            same = got['new', name][buf] == h
            print('%-7s %-44s parent %s parent2 %s new %s%s' % (name, buf, h[:16], got['parent2', name][buf][:16],
                                                              got['new', name][buf][:16],
                                                              '' if stable else '   (parent does not repeat)'))
            if not stable:
                unstable.append('%s %s' % (name, buf))
            elif not same:
                differ.append('%s %s' % (name, buf))
    print('buffers the parent itself does not reproduce (left to the tests\' tolerances): %s' % (unstable or 'none'))
    bad = [u for u in unstable if u.startswith('default fit') or u.endswith('/uc') or u.endswith('/mu_y')]
    if bad:
        differ += ['(must repeat) ' + u for u in bad]
    print('RESULT: %s' % ('every repeatable buffer has the parent\'s bits' if not differ else 'DIFFERENT: %s' % differ))
    return 1 if differ else 0


if __name__ == '__main__':
    sys.exit(main())
