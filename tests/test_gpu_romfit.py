"""gpi_rom_fit (one-launch batched ROM fit) and bottleneck.utils.OptimizeEffectiveProperties on the GPU.

Exact checks (bit for bit): the result of a sample depends on nothing but its own rows and the
scalars -- repeat runs, any split of the batch, any split of the iterations, untouched padding.
First evaluation vs fp64 at the project's ROM bars (1e-5).  Trajectories vs the fp64 restatement
(tests/romfit_ref.py): Adam's eps makes elements with |g| <~ 1e-8 sensitive to the last bits of the
gradient, so the bar is not fixed in advance but taken from the drift D of the module-path loop
(RomOperatorFunction + mse_loss + torch.optim.Adam, fp32 on the GPU) against the same fp64
trajectory: the kernel may drift 3 D (two fp32 evaluations of one gradient with different summation
orders err at the same order, independently), capped at 1e-3 (x) and 1e-4 (J).

Measured on an MI355X (profiles/romfit_parity.txt): see that file for D and the kernel's drift per case."""
import ctypes as C

import numpy as np
import pytest
import torch

from elbo_ref import load, physics, tensor_rel
from oracle import elbo as oelbo
from oracle import fem
import romfit_ref as R

pytestmark = pytest.mark.gpu
GPI_ERR_UNSUPPORTED = -3
SENTINEL = -777.0
CAP_X, CAP_J = 1e-3, 1e-4
_CACHE = {}


def cuda(a, dtype=torch.float32):
    return torch.tensor(np.asarray(a), dtype=dtype, device='cuda')


def synthetic(nc, r, N, seed, noise=0.05):
    """Seeded labels for the (nc, r) ROM: Y = W u(x*) + noise, x* = 0.7 randn, F from random corner data
    (fp64 oracle, rounded to fp32 once: every implementation reads the same numbers)."""
    key = ('syn', nc, r, N, seed, noise)
    if key not in _CACHE:
        M, W, bc = physics(nc, r)
        rng = np.random.default_rng(seed)
        mc = fem.unit_square_mesh(nc)
        F = np.stack([fem.f_rom_bc(mc, u) for u in rng.uniform(-0.5, 0.5, (N, 4))]).astype(np.float32)
        xs = torch.tensor(0.7 * rng.standard_normal((N, M.shape[2])))
        mu, _ = oelbo.rom_operator(torch.tensor(W, dtype=torch.float64), torch.tensor(M, dtype=torch.float64),
                                   torch.tensor(bc), xs, torch.tensor(F, dtype=torch.float64), torch.zeros(W.shape[0]))
        Y = (mu.numpy() + noise * rng.standard_normal(mu.shape)).astype(np.float32)
        _CACHE[key] = (Y, F)
    return _CACHE[key]


def raw_fit(Y, F, nc, r, T, x, m=None, v=None, step0=0, n_total=0, lr=1e-2, sumsq=None, ynorm2=None, x_eval=None,
            uc=None, flag=None, x_stride=None, n=None):
    """gpi_rom_fit on caller-owned buffers; returns the error code."""
    from gpi import _lib as L
    d = L.RomFitDesc()
    d.nc, d.refine, d.n, d.iters, d.n_total = nc, r, Y.shape[0] if n is None else n, T, n_total
    p = lambda t: t.data_ptr() if t is not None else None
    d.Y, d.F, d.x, d.x_stride = p(Y), p(F), p(x), (x_stride if x_stride is not None else x.stride(0) if x is not None else 0)
    d.m, d.v, d.step0 = p(m), p(v), step0
    d.lr, d.beta1, d.beta2, d.eps = lr, 0.9, 0.999, 1e-8
    d.sumsq, d.ynorm2, d.x_eval, d.uc, d.flag = p(sumsq), p(ynorm2), p(x_eval), p(uc), p(flag)
    return L.lib().gpi_rom_fit(C.byref(d), L.stream_handle())


def fit(Y, F, nc, r, T, **kw):
    from gpi.romfit import fit_effective_properties
    return fit_effective_properties(Y, F, nc, r, T, **kw)


def same(a, b):
    return all(torch.equal(getattr(a, k), getattr(b, k)) for k in ('x', 'x_eval', 'uc', 'sumsq', 'ynorm2'))


# ---------------------------------------------------------------- exact checks: nc = 4, r = 2, d_y = 63
@pytest.fixture(scope='module')
def small(device):
    Y, F = synthetic(4, 2, 65, seed=11)
    assert Y.shape == (65, 63)
    return cuda(Y), cuda(F)


def test_two_runs_are_identical(small):
    Y, F = small
    a, b = fit(Y, F, 4, 2, 12), fit(Y, F, 4, 2, 12)
    assert same(a, b) and torch.equal(a.state.m, b.state.m) and torch.equal(a.state.v, b.state.v)
    assert torch.equal(a.objective(), b.objective())
    assert int(a.flag.item()) == 0 and torch.isfinite(a.x).all() and a.x.abs().max() > 0


def test_batch_rows_equal_rows_fitted_alone(small):
    Y, F = small
    whole = fit(Y, F, 4, 2, 12)
    for row in (0, 63, 64):
        one = fit(Y[row:row + 1], F[row:row + 1], 4, 2, 12, n_total=65)
        assert torch.equal(one.x[0], whole.x[row]) and torch.equal(one.sumsq[:, 0], whole.sumsq[:, row])
        assert torch.equal(one.x_eval[0], whole.x_eval[row]) and torch.equal(one.uc[0], whole.uc[row])
        assert torch.equal(one.state.m[0], whole.state.m[row]) and torch.equal(one.state.v[0], whole.state.v[row])
    alone = fit(Y[:1], F[:1], 4, 2, 12)            # n_total = 1: another gradient scale, another trajectory
    assert not torch.equal(alone.x[0], whole.x[0])


def test_continued_fit_equals_one_fit(small):
    Y, F = small
    whole = fit(Y, F, 4, 2, 20)
    first = fit(Y, F, 4, 2, 10)
    second = fit(Y, F, 4, 2, 10, x0=first.x, state=first.state)
    assert second.state.step == 20
    assert torch.equal(second.x, whole.x) and torch.equal(second.x_eval, whole.x_eval)
    assert torch.equal(second.state.m, whole.state.m) and torch.equal(second.state.v, whole.state.v)
    assert torch.equal(torch.cat([first.sumsq, second.sumsq]), whole.sumsq)


def test_x_eval_is_the_x_before_the_last_update(small):
    Y, F = small
    a, b = fit(Y, F, 4, 2, 7), fit(Y, F, 4, 2, 6)
    assert torch.equal(a.x_eval, b.x)
    assert not torch.equal(a.x, b.x)


def test_zero_iterations_and_empty_batch_and_unsupported_nc(small):
    Y, F = small
    x0 = cuda(0.3 * np.random.default_rng(5).standard_normal((65, 32)))
    z = fit(Y, F, 4, 2, 0, x0=x0)
    assert torch.equal(z.x, x0) and z.sumsq.shape == (0, 65)
    assert tensor_rel(z.ynorm2.cpu(), (Y.double() ** 2).sum(1).cpu()) < 1e-14
    e = fit(Y[:0], F[:0], 4, 2, 5)
    assert e.x.shape == (0, 32) and e.sumsq.shape == (5, 0)
    x = torch.zeros(65, 18, device='cuda')
    assert raw_fit(Y, F, 3, 2, 5, x) == GPI_ERR_UNSUPPORTED
    assert torch.equal(x, torch.zeros_like(x))
    assert raw_fit(Y, F, 4, 2, 5, None, n=0) == 0


def test_padding_around_every_output_stays_untouched(small):
    Y, F = small
    N, nt, nn, T, PAD = 65, 32, 25, 6, 16

    def padded(numel, dtype=torch.float32):
        buf = torch.full((numel + 2 * PAD,), SENTINEL, dtype=dtype, device='cuda')
        return buf, buf[PAD:PAD + numel]

    stride = nt + 5
    xb, xv = padded(N * stride)
    x = xv.view(N, stride)
    x[:, :nt] = 0
    bufs = {k: padded(n, dt) for k, n, dt in (('m', N * nt, torch.float32), ('v', N * nt, torch.float32),
                                              ('x_eval', N * nt, torch.float32), ('uc', N * nn, torch.float32),
                                              ('sumsq', T * N, torch.float64), ('ynorm2', N, torch.float64))}
    bufs['m'][1].zero_()
    bufs['v'][1].zero_()
    fb = torch.full((3,), 12345, dtype=torch.int32, device='cuda')
    fb[1] = 0
    assert raw_fit(Y, F, 4, 2, T, x, flag=fb[1:2], **{k: b[1] for k, b in bufs.items()}) == 0
    ref = fit(Y, F, 4, 2, T)
    assert torch.equal(x[:, :nt], ref.x) and torch.equal(bufs['sumsq'][1].view(T, N), ref.sumsq)
    assert torch.equal(bufs['x_eval'][1].view(N, nt), ref.x_eval) and torch.equal(bufs['uc'][1].view(N, nn), ref.uc)
    assert torch.equal(bufs['m'][1].view(N, nt), ref.state.m) and torch.equal(bufs['v'][1].view(N, nt), ref.state.v)
    assert torch.equal(bufs['ynorm2'][1], ref.ynorm2)
    assert (x[:, nt:] == SENTINEL).all() and (xb[:PAD] == SENTINEL).all() and (xb[-PAD:] == SENTINEL).all()
    for k, (b, _) in bufs.items():
        assert (b[:PAD] == SENTINEL).all() and (b[-PAD:] == SENTINEL).all(), k
    assert fb.tolist() == [12345, 0, 12345]
    # without the optional buffers: the same x
    x2 = torch.zeros(N, nt, device='cuda')
    assert raw_fit(Y, F, 4, 2, T, x2) == 0
    assert torch.equal(x2, ref.x)


def test_nan_row_sets_the_flag_and_leaves_the_others(small):
    Y, F = small
    Y4, F4 = Y[:4].clone(), F[:4].clone()
    Y4[1, 17] = float('nan')
    bad = fit(Y4, F4, 4, 2, 8)
    assert int(bad.flag.item()) == 1
    with pytest.raises(Exception, match='non-finite'):
        bad.check()
    keep = [0, 2, 3]
    good = fit(Y4[keep], F4[keep], 4, 2, 8, n_total=4)
    assert int(good.flag.item()) == 0
    assert torch.equal(bad.x[keep], good.x) and torch.equal(bad.sumsq[:, keep], good.sumsq)


# ---------------------------------------------------------------- trajectories vs fp64
def module_loop(Y, F, nc, r, T, lr, marks):
    """What a user of the library without gpi_rom_fit runs: the reference's loop over the native ROM."""
    from gpi.native import RomOperatorFunction
    x = torch.zeros(Y.shape[0], 2 * nc * nc, device='cuda', requires_grad=True)
    opt = torch.optim.Adam([x], lr=lr)
    obj, x_marks = [], {}
    for n in range(T):
        mu, _ = RomOperatorFunction.apply(x, F, nc, r, False)
        J = torch.nn.functional.mse_loss(mu, Y)
        opt.zero_grad()
        J.backward()
        obj.append(J.detach())
        opt.step()
        if n + 1 in marks:
            x_marks[n + 1] = x.detach().clone()
    return {k: v.cpu().numpy() for k, v in x_marks.items()}, torch.stack(obj).double().cpu().numpy()


def kernel_marks(Y, F, nc, r, lr, marks):
    """x after every mark, by continuing one fit from mark to mark (bit-identical to a single fit)."""
    x_marks, sumsq, res, done = {}, [], None, 0
    for n in marks:
        res = fit(Y, F, nc, r, n - done, lr=lr, x0=None if res is None else res.x,
                  state=None if res is None else res.state)
        x_marks[n], done = res.x.cpu().numpy(), n
        sumsq.append(res.sumsq)
    assert int(res.flag.item()) == 0
    return x_marks, torch.cat(sumsq), res


CASES = {
    'c32': dict(nc=4, r=8, N=6, lr=1e-2, T=300),
    'c64': dict(nc=8, r=8, N=8, lr=1e-2, T=300),
    'c64_realisable': dict(nc=8, r=8, N=8, lr=5e-2, T=300),
    'nc4_r32': dict(nc=4, r=32, N=3, lr=1e-2, T=5),
    'nc8_r1': dict(nc=8, r=1, N=3, lr=1e-2, T=5),
}


def case_inputs(name):
    c = CASES[name]
    if name == 'c32':
        d = load('rom_c32.npz')
        return d['Y'], d['F']
    if name == 'c64':
        d = load('rom_c64.npz')
        return d['Y'][:8], d['F'][:8]
    if name == 'c64_realisable':
        return synthetic(8, 8, 8, seed=21, noise=0.0)
    # the refine sweep: labels a fixture's distance from the ROM's range (rom_c32 / rom_c64 draw Y ~ N(0, 0.3)), so
    # that |g| >> Adam's eps as in the fixture cases.  (With near-realisable labels, noise 0.05, some gradients
    # of the 63-label nc = 8, r = 1 problem come within eps and the module-path loop itself drifts 3.3e-3 from
    # fp64 in 5 steps, the kernel 3.4e-3: above the cap that guards against a broken reference path.)
    return synthetic(c['nc'], c['r'], c['N'], seed=31, noise=0.3)


def reference(name):
    """The fp64 trajectory of a case (computed once, shared)."""
    if ('ref', name) not in _CACHE:
        c = CASES[name]
        Y, F = case_inputs(name)
        M, W, bc = physics(c['nc'], c['r'])
        marks = tuple(n for n in R.MARKS if n <= c['T']) + ((c['T'],) if c['T'] not in R.MARKS else ())
        _CACHE[('ref', name)] = (R.fit(W, M, bc, Y, F, c['T'], c['lr'], marks=marks), marks, W)
    return _CACHE[('ref', name)]


@pytest.mark.parametrize('name', list(CASES))
def test_first_evaluation_matches_fp64(device, name):
    c = CASES[name]
    Y, F = case_inputs(name)
    ref, _, _ = reference(name)
    res = fit(cuda(Y), cuda(F), c['nc'], c['r'], 1)
    e_y = tensor_rel(res.ynorm2.cpu(), ref['ynorm2'])
    e_s = tensor_rel((res.sumsq[0] / res.ynorm2).cpu(), ref['sumsq'][0] / ref['ynorm2'])
    print('%s: ynorm2 %.2e, sumsq[0] / ynorm2 %.2e' % (name, e_y, e_s))
    assert e_y < 1e-12 and e_s < 1e-5
    assert torch.equal(res.x_eval, torch.zeros_like(res.x_eval))


@pytest.mark.parametrize('name', list(CASES))
def test_trajectory_within_three_times_the_module_path_drift(device, name):
    c = CASES[name]
    Y, F = case_inputs(name)
    ref, marks, _ = reference(name)
    Yd, Fd = cuda(Y), cuda(F)
    mx, mobj = module_loop(Yd, Fd, c['nc'], c['r'], c['T'], c['lr'], marks)
    kx, ksumsq, res = kernel_marks(Yd, Fd, c['nc'], c['r'], c['lr'], marks)
    kobj = (ksumsq.sum(1) / float(Y.shape[0] * Y.shape[1])).cpu().numpy()
    Dx, Dj = R.x_drift(mx, ref['x_marks']), R.j_drift(mobj, ref['objective'])
    Kx, Kj = R.x_drift(kx, ref['x_marks']), R.j_drift(kobj, ref['objective'])
    print('%s: J %.3e -> %.3e | x drift: module path D %.2e, kernel %.2e | J drift: module path D %.2e, kernel %.2e'
          % (name, ref['objective'][0], ref['objective'][-1], Dx, Kx, Dj, Kj))
    assert Kx <= min(3 * Dx, CAP_X), (Kx, Dx)
    assert Kj <= min(3 * Dj, CAP_J), (Kj, Dj)
    # the single T-iteration launch is the chain of continued launches, bit for bit
    whole = fit(Yd, Fd, c['nc'], c['r'], c['T'], lr=c['lr'])
    assert torch.equal(whole.x, res.x) and torch.equal(whole.sumsq, ksumsq)
    assert torch.equal(whole.objective().cpu(), torch.tensor(kobj))


# ---------------------------------------------------------------- the reference-signature wrapper
class _DS(object):
    def __init__(self, **t):
        self.t = t

    def get(self, key, random_subset=None):
        return self.t[key]


def operator(nc, r):
    from bottleneck.ROM import ROM
    from bottleneck.components import ReducedOrderModelOperator
    from physics.grid import StructuredGrid
    W = torch.tensor(physics(nc, r)[1], dtype=torch.float32)
    return ReducedOrderModelOperator(ROM(StructuredGrid(nc), r), W, dtype=torch.float32, device='cuda')


def test_optimize_effective_properties_first_prediction(device):
    """Y_predict of a T = 1 fit is forward_mean at logX = 0: vs fp64 at the ROM operator's bar."""
    from bottleneck.utils import OptimizeEffectiveProperties
    Y, F = case_inputs('c64')
    ref, _, _ = reference('c64')
    M, W, bc = physics(8, 8)
    one = R.fit(W, M, bc, Y, F, 1, 1e-2)
    logX, Yp, obj, rel = OptimizeEffectiveProperties(_DS(Y=cuda(Y), F_ROM_BC=cuda(F)), operator(8, 8),
                                                     num_iterations=1, verbose=False)
    assert tensor_rel(Yp.cpu(), one['Y_predict']) < 1e-5
    assert len(obj) == 1 and rel == [] and abs(obj[0] - ref['objective'][0]) < 1e-5 * ref['objective'][0]
    # (x after the step is Adam's eps-sensitive quotient already: held to the cap of every fp32 path)
    assert logX.requires_grad and tensor_rel(logX.detach().cpu(), one['x']) <= CAP_X


def test_optimize_effective_properties_vs_reference_run(device):
    """The reference's own run (romfit_c32.npz: N = 6, T = 201, fp32 CPU) at the trajectory bars of the c32
    case: outputs, objective history (length and values) and the logged relative errors."""
    from bottleneck.utils import OptimizeEffectiveProperties
    g = load('romfit_c32.npz')
    Y, F = case_inputs('c32')
    ref, marks, _ = reference('c32')
    T = int(g['T'])
    Yd, Fd = cuda(Y), cuda(F)
    mx, mobj = module_loop(Yd, Fd, 4, 8, T, 1e-2, (T,))
    M, W, bc = physics(4, 8)
    r64 = R.fit(W, M, bc, Y, F, T, 1e-2, marks=(T,))
    bar_x = min(3 * R.x_drift(mx, r64['x_marks']), CAP_X)
    bar_j = min(3 * R.j_drift(mobj, r64['objective']), CAP_J)
    logX, Yp, obj, rel = OptimizeEffectiveProperties(_DS(Y=Yd, F_ROM_BC=Fd), operator(4, 8), num_iterations=T,
                                                     verbose=False)
    errs = dict(x=tensor_rel(logX.detach().cpu(), g['logX']), Y_predict=tensor_rel(Yp.cpu(), g['Y_predict']),
                objective=R.j_drift(obj, g['objective']), relerr=tensor_rel(rel, g['relerr_list']))
    print('vs the reference run: %s | bars x %.2e, J %.2e' % (errs, bar_x, bar_j))
    assert len(obj) == T == len(g['objective']) and len(rel) == len(g['relerr_list']) == 2
    assert errs['x'] <= bar_x and errs['Y_predict'] <= bar_x
    assert errs['objective'] <= bar_j and errs['relerr'] <= bar_j


def test_optimize_effective_properties_module_path_branch(device):
    """With a y_preprocessor the same loop runs through forward_mean (gpi_rom) + torch Adam on the device.
    An identity preprocessor lands on the fp64 fit within the caps every fp32 path is held to."""
    from bottleneck.utils import OptimizeEffectiveProperties
    Y, F = case_inputs('nc8_r1')
    ref, _, _ = reference('nc8_r1')
    logX, Yp, obj, rel = OptimizeEffectiveProperties(_DS(Y=cuda(Y), F_ROM_BC=cuda(F)), operator(8, 1), num_iterations=5,
                                                     verbose=False, y_preprocessor=lambda y: y)
    assert logX.requires_grad and Yp.shape == Y.shape and Yp.is_cuda and rel == [] and len(obj) == 5
    assert tensor_rel(logX.detach().cpu(), ref['x']) <= CAP_X
    assert R.j_drift(obj, ref['objective']) <= CAP_J
