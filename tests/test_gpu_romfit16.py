"""gpi_rom_fit at nc = 16 (rom_fit_kernel<16>) and OptimizeEffectiveProperties on the 16 x 16 coarse mesh.

The checks of tests/test_gpu_romfit.py on the smallest shapes at which the nc = 16 kernel can go wrong:
r = 1 (d_y = 255: every fine node is a coarse node, the i0 / rows edge cases of the setup), r = 2
(d_y = 1023) and, for the first evaluation only, r = 8 (d_y = 16383).  Labels Y = W u(x*) + 0.3 randn.

Exact checks (bit for bit): a sample's result depends on its own rows and the scalars alone.  First
evaluation vs fp64 at the project's ROM bar (1e-5).  Trajectory vs the fp64 restatement with the sparse
stiffness tensor (tests/romfit16_ref.py): the kernel may drift 3 D, D the module-path loop's drift
(RomOperatorFunction + mse_loss + torch.optim.Adam, fp32 on the GPU), capped at 1e-3 (x) and 1e-4 (J).

The cap is a condition the reference path must meet alone, so the case was fixed on the CPU, before any GPU
run, from the sparse restatement in fp32 against fp64 (r = 2, N = 3, noise 0.3, lr 1e-2): it has to stay
within a third of each cap (3.3e-4 on x, 3.3e-5 on J) at the largest T of 300 / 100 / 50 / 20.  On the
16 x 16 mesh label noise 0.3 does NOT put every |g| far above Adam's eps: of the 1536 gradient elements at
x = 0 the median is 1e-6 but the smallest are 1e-9 .. 1e-11 at every seed, and the first updates of those
elements carry the last bits of the gradient.  The x drift is therefore set at the first marks and does not
depend on T (J: <= 1.9e-7 everywhere), and it depends on the draw: seeds 31 .. 36 give 6.0e-4, 2.8e-3,
6.0e-4, 1.2e-3, 1.1e-3, 8.7e-4 (above a third of the cap at every T), seed 37 gives 3.30e-4 at T = 300, 100,
50 and 20 alike.  Hence SEED = 37 (the first seed from 31 upward that meets the condition) and T = 300.
The condition is a property of the labels, not of one fp32 path: at seed 31 the module-path loop on the GPU
drifts D = 1.01e-3 (over the cap by itself) and the kernel 1.02e-3; at seed 37, D = 2.5e-4 and the kernel
2.2e-4.  Measured D and the kernel's drift, per mark: profiles/romfit16_parity.txt."""
import ctypes as C

import numpy as np
import pytest
import torch

from elbo_ref import physics, tensor_rel
import romfit16_ref as R16
import romfit_ref as R

pytestmark = pytest.mark.gpu
GPI_ERR_UNSUPPORTED = -3
SENTINEL = -777.0
CAP_X, CAP_J = 1e-3, 1e-4
NC, NT, NN = 16, 512, 289
T_TRAJ, LR, SEED = 300, 1e-2, 37
_CACHE = {}


def cuda(a, dtype=torch.float32):
    return torch.tensor(np.asarray(a), dtype=dtype, device='cuda')


def synthetic(nc, r, N, seed, noise=0.3):
    """Seeded labels for the (nc, r) ROM (romfit16_ref.synthetic_labels), computed once per shape."""
    key = ('syn', nc, r, N, seed, noise)
    if key not in _CACHE:
        _CACHE[key] = R16.synthetic_labels(nc, r, N, seed, noise)
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


# ---------------------------------------------------------------- exact checks: nc = 16, r = 2, d_y = 1023
@pytest.fixture(scope='module')
def small(device):
    Y, F = synthetic(NC, 2, 5, seed=11)
    assert Y.shape == (5, 1023)
    return cuda(Y), cuda(F)


def test_two_runs_are_identical(small):
    Y, F = small
    a, b = fit(Y, F, NC, 2, 12), fit(Y, F, NC, 2, 12)
    assert same(a, b) and torch.equal(a.state.m, b.state.m) and torch.equal(a.state.v, b.state.v)
    assert torch.equal(a.objective(), b.objective())
    assert int(a.flag.item()) == 0 and torch.isfinite(a.x).all() and a.x.abs().max() > 0
    assert torch.isfinite(a.sumsq).all() and (a.sumsq > 0).all() and a.objective()[-1] < a.objective()[0]


def test_batch_rows_equal_rows_fitted_alone(small):
    Y, F = small
    whole = fit(Y, F, NC, 2, 12)
    for row in (0, 3, 4):
        one = fit(Y[row:row + 1], F[row:row + 1], NC, 2, 12, n_total=5)
        assert torch.equal(one.x[0], whole.x[row]) and torch.equal(one.sumsq[:, 0], whole.sumsq[:, row])
        assert torch.equal(one.x_eval[0], whole.x_eval[row]) and torch.equal(one.uc[0], whole.uc[row])
        assert torch.equal(one.state.m[0], whole.state.m[row]) and torch.equal(one.state.v[0], whole.state.v[row])
    alone = fit(Y[:1], F[:1], NC, 2, 12)           # n_total = 1: another gradient scale, another trajectory
    assert not torch.equal(alone.state.m[0], whole.state.m[0])


def test_continued_fit_equals_one_fit(small):
    Y, F = small
    whole = fit(Y, F, NC, 2, 12)
    first = fit(Y, F, NC, 2, 6)
    second = fit(Y, F, NC, 2, 6, x0=first.x, state=first.state)
    assert second.state.step == 12
    assert torch.equal(second.x, whole.x) and torch.equal(second.x_eval, whole.x_eval)
    assert torch.equal(second.uc, whole.uc)
    assert torch.equal(second.state.m, whole.state.m) and torch.equal(second.state.v, whole.state.v)
    assert torch.equal(torch.cat([first.sumsq, second.sumsq]), whole.sumsq)


def test_x_eval_is_the_x_before_the_last_update(small):
    Y, F = small
    a, b = fit(Y, F, NC, 2, 7), fit(Y, F, NC, 2, 6)
    assert torch.equal(a.x_eval, b.x)
    assert not torch.equal(a.x, b.x)


def test_zero_iterations_and_empty_batch_and_unsupported_nc(small):
    Y, F = small
    x0 = cuda(0.3 * np.random.default_rng(5).standard_normal((5, NT)))
    z = fit(Y, F, NC, 2, 0, x0=x0)
    assert torch.equal(z.x, x0) and z.sumsq.shape == (0, 5)
    assert tensor_rel(z.ynorm2.cpu(), (Y.double() ** 2).sum(1).cpu()) < 1e-14
    e = fit(Y[:0], F[:0], NC, 2, 5)
    assert e.x.shape == (0, NT) and e.sumsq.shape == (5, 0)
    assert raw_fit(Y, F, NC, 2, 5, None, n=0) == 0
    x = torch.full((5, 2 * 12 * 12), SENTINEL, device='cuda')
    assert raw_fit(Y, F, 12, 2, 5, x) == GPI_ERR_UNSUPPORTED
    assert (x == SENTINEL).all()


def test_padding_around_every_output_stays_untouched(small):
    Y, F = small
    N, T, PAD = 5, 6, 16

    def padded(numel, dtype=torch.float32):
        buf = torch.full((numel + 2 * PAD,), SENTINEL, dtype=dtype, device='cuda')
        return buf, buf[PAD:PAD + numel]

    stride = NT + 5
    xb, xv = padded(N * stride)
    x = xv.view(N, stride)
    x[:, :NT] = 0
    bufs = {k: padded(n, dt) for k, n, dt in (('m', N * NT, torch.float32), ('v', N * NT, torch.float32),
                                              ('x_eval', N * NT, torch.float32), ('uc', N * NN, torch.float32),
                                              ('sumsq', T * N, torch.float64), ('ynorm2', N, torch.float64))}
    bufs['m'][1].zero_()
    bufs['v'][1].zero_()
    fb = torch.full((3,), 12345, dtype=torch.int32, device='cuda')
    fb[1] = 0
    assert raw_fit(Y, F, NC, 2, T, x, flag=fb[1:2], **{k: b[1] for k, b in bufs.items()}) == 0
    ref = fit(Y, F, NC, 2, T)
    assert torch.equal(x[:, :NT], ref.x) and torch.equal(bufs['sumsq'][1].view(T, N), ref.sumsq)
    assert torch.equal(bufs['x_eval'][1].view(N, NT), ref.x_eval) and torch.equal(bufs['uc'][1].view(N, NN), ref.uc)
    assert torch.equal(bufs['m'][1].view(N, NT), ref.state.m) and torch.equal(bufs['v'][1].view(N, NT), ref.state.v)
    assert torch.equal(bufs['ynorm2'][1], ref.ynorm2)
    assert (x[:, NT:] == SENTINEL).all() and (xb[:PAD] == SENTINEL).all() and (xb[-PAD:] == SENTINEL).all()
    for k, (b, _) in bufs.items():
        assert (b[:PAD] == SENTINEL).all() and (b[-PAD:] == SENTINEL).all(), k
    assert fb.tolist() == [12345, 0, 12345]
    # without the optional buffers: the same x
    x2 = torch.zeros(N, NT, device='cuda')
    assert raw_fit(Y, F, NC, 2, T, x2) == 0
    assert torch.equal(x2, ref.x)


def test_nan_row_sets_the_flag_and_leaves_the_others(small):
    Y, F = small
    Y4, F4 = Y[:4].clone(), F[:4].clone()
    Y4[1, 517] = float('nan')
    bad = fit(Y4, F4, NC, 2, 8)
    assert int(bad.flag.item()) == 1
    with pytest.raises(Exception, match='non-finite'):
        bad.check()
    keep = [0, 2, 3]
    good = fit(Y4[keep], F4[keep], NC, 2, 8, n_total=4)
    assert int(good.flag.item()) == 0
    assert torch.equal(bad.x[keep], good.x) and torch.equal(bad.sumsq[:, keep], good.sumsq)
    assert torch.equal(bad.uc[keep], good.uc) and torch.equal(bad.state.v[keep], good.state.v)


# ---------------------------------------------------------------- vs fp64
def inputs(r):
    return synthetic(NC, r, 3, seed=SEED)


def reference(r, T, marks=()):
    """The fp64 fit of inputs(r) (computed once, shared)."""
    if ('ref', r, T) not in _CACHE:
        Y, F = inputs(r)
        M, W, bc = physics(NC, r)
        _CACHE[('ref', r, T)] = R16.fit(W, M, bc, Y, F, T, LR, marks=marks)
    return _CACHE[('ref', r, T)]


@pytest.mark.parametrize('r', [1, 2, 8])
def test_first_evaluation_matches_fp64(device, r):
    Y, F = inputs(r)
    assert Y.shape == (3, (NC * r + 1) * (NC * r - 1))
    ref = reference(r, 1)
    res = fit(cuda(Y), cuda(F), NC, r, 1)
    e_y = tensor_rel(res.ynorm2.cpu(), ref['ynorm2'])
    e_s = tensor_rel((res.sumsq[0] / res.ynorm2).cpu(), ref['sumsq'][0] / ref['ynorm2'])
    print('nc 16, r = %d: ynorm2 %.2e, sumsq[0] / ynorm2 %.2e' % (r, e_y, e_s))
    assert e_y < 1e-12 and e_s < 1e-5
    assert torch.equal(res.x_eval, torch.zeros_like(res.x_eval)) and int(res.flag.item()) == 0


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


def test_trajectory_within_three_times_the_module_path_drift(device):
    T = T_TRAJ
    Y, F = inputs(2)
    marks = tuple(n for n in R.MARKS if n <= T) + ((T,) if T not in R.MARKS else ())
    ref = reference(2, T, marks)
    Yd, Fd = cuda(Y), cuda(F)
    mx, mobj = module_loop(Yd, Fd, NC, 2, T, LR, marks)
    kx, ksumsq, res = kernel_marks(Yd, Fd, NC, 2, LR, marks)
    kobj = (ksumsq.sum(1) / float(Y.shape[0] * Y.shape[1])).cpu().numpy()
    Dx, Dj = R.x_drift(mx, ref['x_marks']), R.j_drift(mobj, ref['objective'])
    Kx, Kj = R.x_drift(kx, ref['x_marks']), R.j_drift(kobj, ref['objective'])
    print('nc 16, r = 2, T = %d: J %.3e -> %.3e | x drift: module path D %.2e, kernel %.2e | J drift: module path '
          'D %.2e, kernel %.2e' % (T, ref['objective'][0], ref['objective'][-1], Dx, Kx, Dj, Kj))
    assert Kx <= min(3 * Dx, CAP_X), (Kx, Dx)
    assert Kj <= min(3 * Dj, CAP_J), (Kj, Dj)
    # the single T-iteration launch is the chain of continued launches, bit for bit
    whole = fit(Yd, Fd, NC, 2, T, lr=LR)
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


def counted(monkeypatch):
    from gpi import romfit
    calls, inner = [], romfit.fit_effective_properties

    def spy(*a, **kw):
        calls.append(a[2:5])
        return inner(*a, **kw)

    monkeypatch.setattr(romfit, 'fit_effective_properties', spy)
    return calls


def test_optimize_effective_properties_takes_the_one_launch_path(device, monkeypatch):
    from bottleneck.utils import OptimizeEffectiveProperties
    Y, F = inputs(2)
    one = reference(2, 1)
    calls = counted(monkeypatch)
    ds = _DS(Y=cuda(Y), F_ROM_BC=cuda(F))
    logX, Yp, obj, rel = OptimizeEffectiveProperties(ds, operator(NC, 2), num_iterations=1, verbose=False)
    assert calls == [(NC, 2, 1)]
    assert tensor_rel(Yp.cpu(), one['Y_predict']) < 1e-5
    assert len(obj) == 1 and rel == [] and abs(obj[0] - one['objective'][0]) < 1e-5 * one['objective'][0]
    assert logX.requires_grad and logX.shape == (3, NT)
    logX, Yp, obj, rel = OptimizeEffectiveProperties(ds, operator(NC, 2), num_iterations=7, verbose=False)
    assert len(calls) == 2 and len(obj) == 7 and logX.requires_grad and obj[-1] < obj[0]


def test_optimize_effective_properties_module_path_with_a_preprocessor(device, monkeypatch):
    from bottleneck.utils import OptimizeEffectiveProperties
    Y, F = inputs(2)
    calls = counted(monkeypatch)
    logX, Yp, obj, rel = OptimizeEffectiveProperties(_DS(Y=cuda(Y), F_ROM_BC=cuda(F)), operator(NC, 2),
                                                     num_iterations=2, verbose=False, y_preprocessor=lambda y: y)
    assert calls == []
    assert logX.requires_grad and Yp.shape == Y.shape and len(obj) == 2
