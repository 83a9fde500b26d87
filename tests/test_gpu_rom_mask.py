"""Observation weights in gpi_rom's fused log-likelihood (gpi_rom_desc.y_weight / yw_stride), operator level,
in every kernel form that serves GPI_ROM_LOGLIK: rom_kernel_fast at nc = 4, 8, 16 and the generic rom_kernel
(nc = 5, which no native form takes).

Against fp64 (tests/partial_ref.rom_loglik) at the bars of test_rom_*: the value 1e-5, gx and the per-sample
d/dlogsigma_y rows 1e-4 (tensor_rel: max|g - ref| / max|ref|).  Exactly: all-ones weights equal a launch without
weights, a shared row equals per-sample copies of it, holes filled with NaN equal holes filled with 0, a
sample's outputs do not depend on its batch mates, all-zero weights give 0, and rows past n stay untouched.

Inputs have the statistics of test_gpu_rom16.py: x ~ N(0.3, 0.7^2), Dirichlet values U(-0.5, 0.5), logsigma_y =
log 0.3 + 0.1 eps, Y = mu_fp64 + 0.3 eps.  Shapes: the smallest with more than one sample, a ragged last batch
of prefetched nodes and several fine nodes per coarse square in each form."""
import ctypes as C

import numpy as np
import pytest
import torch

from elbo_ref import physics, tensor_rel
import partial_ref as P

pytestmark = pytest.mark.gpu

GPI_ERR_ARG = -1
SENTINEL = -777.0
SHAPES = [(4, 8, 3), (8, 4, 5), (16, 2, 3), (5, 4, 2)]          # (nc, r, N); nc = 5: the generic kernel
MASKS = ['rand30', 'square', 'single', 'zeros']
_REF = {}


def cuda(a, dtype=torch.float32):
    return torch.tensor(np.asarray(a), dtype=dtype, device='cuda')


def case(nc, r, N):
    """Seeded fp32 inputs of a shape, computed once."""
    key = (nc, r, N)
    if key not in _REF:
        rng = np.random.default_rng(1000 + 37 * nc + r)
        n = nc * r
        nn, nt, dy = (nc + 1) ** 2, 2 * nc * nc, (n + 1) * (n - 1)
        x = rng.normal(0.3, 0.7, (N, nt)).astype(np.float32)
        F = np.zeros((N, nn), dtype=np.float32)
        bn = [e for e in range(nn) if e % (nc + 1) in (0, nc)]
        F[:, bn] = rng.uniform(-0.5, 0.5, (N, len(bn)))
        ls = (np.log(0.3) + 0.1 * rng.normal(size=dy)).astype(np.float32)
        _, mu, _, _ = P.rom_loglik(nc, r, x, F, np.zeros((N, dy)), ls, None)
        Y = (mu + 0.3 * rng.normal(size=(N, dy))).astype(np.float32)
        # the 'single' mask's node: Y two standard deviations off the fp64 mean there, so that the one-term value
        # -1/2 (2 ls + 4 + log 2 pi) ~ -1.7 is no near-cancellation of its three summands
        p1 = (n // 2 + 1) * (n - 1) + n // 3
        Y[:, p1] = (mu[:, p1] + 2 * np.exp(ls[p1].astype(np.float64))).astype(np.float32)
        _REF[key] = dict(nc=nc, r=r, N=N, n=n, nn=nn, nt=nt, dy=dy, x=x, F=F, ls=ls, Y=Y, mu=mu, p1=p1, masks={}, ref={})
    return _REF[key]


def mask_of(c, kind):
    """[N, d_y] float32 0/1 (kept per case).  rand30: seeded, 30 % observed, another set per sample.  square: every
    fine node of one interior coarse square (its edges included) unobserved.  single: one observed node (case()'s
    p1).  zeros: nothing observed."""
    if kind not in c['masks']:
        N, dy, n, r, nc = c['N'], c['dy'], c['n'], c['r'], c['nc']
        rng = np.random.default_rng(7 + len(kind))
        if kind == 'rand30':
            w = (rng.random((N, dy)) < 0.3).astype(np.float32)
        elif kind == 'square':
            w = np.ones((n + 1, n - 1), dtype=np.float32)
            I, J = 1, nc - 2
            w[J * r:(J + 1) * r + 1, I * r - 1:(I + 1) * r] = 0          # rows j, columns i - 1
            assert w.sum() < w.size
            w = np.repeat(w.reshape(1, dy), N, 0)
        elif kind == 'single':
            w = np.zeros((N, dy), dtype=np.float32)
            w[:, c['p1']] = 1
        else:
            w = np.zeros((N, dy), dtype=np.float32)
        c['masks'][kind] = w
    return c['masks'][kind]


def ref_of(c, kind):
    if kind not in c['ref']:
        w = mask_of(c, kind)
        c['ref'][kind] = P.rom_loglik(c['nc'], c['r'], c['x'], c['F'], c['Y'], c['ls'], w)
    return c['ref'][kind]


def launch(c, w=None, shared=False, part=True, Y=None, rows=None, pad=0, mode=None, yw_stride=None, check=True):
    """One gpi_rom launch on case c (rows: a sample subset) -> dict(gx, g, acc, mu, rc).  w [N, d_y] numpy or
    None; shared: pass its first row with yw_stride 0.  pad: extra sentinel rows behind every output."""
    from gpi import _lib as L
    sel = slice(None) if rows is None else rows
    x, F, ls = cuda(c['x'][sel]), cuda(c['F'][sel]), cuda(c['ls'])
    Yt = cuda((c['Y'] if Y is None else Y)[sel])
    N = x.shape[0]
    gx = torch.full((N + pad, c['nt']), SENTINEL, device='cuda')
    mu = torch.full((N + pad, c['dy']), SENTINEL, device='cuda')
    acc = torch.zeros(L.GPI_REPLICAS, dtype=torch.float64, device='cuda')
    d = L.RomDesc()
    d.nc, d.refine, d.n, d.mode = c['nc'], c['r'], N, L.ROM_LOGLIK if mode is None else mode
    d.x, d.x_stride, d.F, d.Y, d.logsig_y = x.data_ptr(), c['nt'], F.data_ptr(), Yt.data_ptr(), ls.data_ptr()
    d.gx, d.gx_stride, d.mu_y, d.loss_acc, d.loss_scale = gx.data_ptr(), c['nt'], mu.data_ptr(), acc.data_ptr(), 1.0
    if mode is not None:
        d.dmu = mu.data_ptr()
    if part:
        g = torch.full((N + pad, c['dy']), SENTINEL, device='cuda')
        d.gls_part = g.data_ptr()
    else:
        g = torch.zeros(c['dy'], dtype=torch.float64, device='cuda')
        d.gacc_logsig = g.data_ptr()
    wt = None
    if w is not None:
        wt = cuda(w[0] if shared else w[sel])
        d.y_weight = wt.data_ptr()
        d.yw_stride = (0 if shared else c['dy']) if yw_stride is None else yw_stride
    rc = L.lib().gpi_rom(C.byref(d), L.stream_handle())
    torch.cuda.synchronize()
    if check:
        assert rc == 0, rc
    return dict(gx=gx, g=g, acc=acc, mu=mu, rc=rc)


def same(a, b, keys=('gx', 'g', 'acc', 'mu')):
    return all(torch.equal(a[k], b[k]) for k in keys)


@pytest.mark.parametrize('nc,r,N', SHAPES)
@pytest.mark.parametrize('kind', MASKS)
def test_masked_loglik_against_fp64(device, nc, r, N, kind):
    c = case(nc, r, N)
    w = mask_of(c, kind)
    L_ref, mu_ref, gx_ref, gls_ref = ref_of(c, kind)
    for part in (True, False):
        o = launch(c, w, part=part)
        val = o['acc'].sum().item()
        rows = o['g'].cpu().numpy() if part else None
        assert tensor_rel(o['mu'].cpu(), mu_ref) < 1e-5                # mu_y is written at every node
        if kind == 'zeros':
            assert val == 0.0
            assert torch.count_nonzero(o['gx']).item() == 0 and torch.count_nonzero(o['g']).item() == 0
            continue
        e_L = abs(val - L_ref) / abs(L_ref)
        e_gx = tensor_rel(o['gx'].cpu(), gx_ref)
        e_g = tensor_rel(rows, gls_ref) if part else tensor_rel(o['g'].cpu(), gls_ref.sum(0))
        print('nc %d r %d N %d %s %s: L %.2e gx %.2e gls %.2e' % (nc, r, N, kind, 'rows' if part else 'atomics',
                                                                 e_L, e_gx, e_g))
        assert e_L <= 1e-5
        assert e_gx < 1e-4
        assert e_g < 1e-4
        if part:                                                      # unobserved entries: exact zeros
            assert np.all(rows[w == 0] == 0)


@pytest.mark.parametrize('nc,r,N', SHAPES)
def test_exact_properties(device, nc, r, N):
    c = case(nc, r, N)
    ones = np.ones((N, c['dy']), dtype=np.float32)
    w = mask_of(c, 'rand30')
    for part in (True, False):
        plain = launch(c, None, part=part)
        # all-ones weights, shared or per sample: the launch without weights
        assert same(launch(c, ones, part=part), plain)
        assert same(launch(c, ones, shared=True, part=part), plain)
        # a shared row: per-sample copies of it
        rep = np.repeat(w[:1], N, 0)
        a = launch(c, rep, part=part)
        assert same(launch(c, rep, shared=True, part=part), a)
        # holes hold NaN / Inf: what they hold is never read into a result
        m = launch(c, w, part=part)
        Yn = c['Y'].copy()
        Yn[w == 0] = np.nan
        Yn[0, np.flatnonzero(w[0] == 0)[:3]] = np.inf
        h = launch(c, w, part=part, Y=Yn)
        assert same(h, m)
        assert torch.isfinite(h['gx']).all() and torch.isfinite(h['g']).all() and torch.isfinite(h['acc']).all()
    # a sample's outputs do not depend on its batch mates (N <= GPI_REPLICAS: a loss replica per sample)
    m = launch(c, w, part=True)
    for s in range(N):
        one = launch(c, w, part=True, rows=slice(s, s + 1))
        assert torch.equal(one['gx'][0], m['gx'][s]) and torch.equal(one['g'][0], m['g'][s])
        assert torch.equal(one['mu'][0], m['mu'][s]) and one['acc'][0].item() == m['acc'][s].item()


@pytest.mark.parametrize('nc,r,N', SHAPES)
def test_rows_past_n_stay_untouched(device, nc, r, N):
    c = case(nc, r, N)
    o = launch(c, mask_of(c, 'rand30'), part=True, pad=2)
    for k in ('gx', 'g', 'mu'):
        assert torch.all(o[k][N:] == SENTINEL), k
        assert not torch.any(o[k][:N] == SENTINEL), k


@pytest.mark.parametrize('nc,r,N', SHAPES)
def test_misused_weights_are_refused(device, nc, r, N):
    from gpi import _lib as L
    c = case(nc, r, N)
    w = mask_of(c, 'rand30')
    for bad in (1, c['dy'] - 1, c['dy'] + 1, -c['dy']):
        o = launch(c, w, yw_stride=bad, check=False)
        assert o['rc'] == GPI_ERR_ARG
        assert torch.all(o['gx'] == SENTINEL) and torch.all(o['g'] == SENTINEL)
    for mode in (L.ROM_FORWARD, L.ROM_BACKWARD):
        o = launch(c, w, mode=mode, check=False)
        assert o['rc'] == GPI_ERR_ARG
        assert torch.all(o['gx'] == SENTINEL)
