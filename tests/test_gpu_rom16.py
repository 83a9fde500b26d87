"""The 16 x 16 coarse-grained model (gpi_rom at nc = 16: 255 interior unknowns, bandwidth 15; rom.hip's
chol16_wave / band_sweep16 inside rom_kernel_fast<16> and rom16_coarse_kernel) against the fp64 oracle
(oracle/elbo.py: the reference's dense K = M x^T, row-replaced Dirichlet rows, dense solve), through
every mode and option of gpi_rom_desc and every user of the launch up to the fused training step.

Bars are the project's nc = 8 bars: mu / u_c 1e-5, log-likelihood 1e-5, d/dx 1e-4, d/dlogsigma_y 1e-5
(tensor_rel: max|g - ref| / max|ref| over the whole tensor).  Inputs have the statistics of the nc = 8
tests: x ~ N(0.3, 0.7^2), Dirichlet values U(-0.5, 0.5) at every boundary node, logsigma_y =
log 0.3 + 0.1 eps, Y = mu_fp64 + 0.3 eps.  Shapes: r = 1 (fine grid = coarse grid, d_y = 255), r = 2
(32^2), r = 8 once (128^2, the real square size); N in {1, 3, 70} for the workgroup-per-sample form,
N = 200 and 1 for the wave-per-sample coarse-only form (two samples per workgroup: ragged at N = 1)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, PKG
from elbo_ref import physics, oracle_elbo, tensor_rel, check_grads
from oracle import codec as ocodec
from oracle import elbo as oelbo

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
NC = 16
NN = (NC + 1) ** 2
NT2 = 2 * NC * NC
BNODES = [e for e in range(NN) if e % (NC + 1) in (0, NC)]
_REF = {}


def cuda(a, dtype=torch.float32):
    return torch.tensor(np.asarray(a), dtype=dtype, device='cuda')


def t64(a, grad=False):
    return torch.tensor(np.asarray(a), dtype=torch.float64, requires_grad=grad)


def inputs(r, N, seed):
    """fp32 inputs (as float32 arrays) of one case, without the targets."""
    rng = np.random.default_rng(seed)
    n = NC * r
    dy = (n + 1) * (n - 1)
    x = rng.normal(0.3, 0.7, (N, NT2)).astype(np.float32)
    F = np.zeros((N, NN), dtype=np.float32)
    F[:, BNODES] = rng.uniform(-0.5, 0.5, (N, len(BNODES)))
    ls = (np.log(0.3) + 0.1 * rng.normal(size=dy)).astype(np.float32)
    return rng, x, F, ls, dy


def ref_case(r, N, seed):
    """Inputs and the fp64 oracle's mu, u_c, log-likelihood L, d(-L)/dx and d(-L)/dlogsigma_y, computed once."""
    key = (r, N, seed)
    if key not in _REF:
        rng, x, F, ls, dy = inputs(r, N, seed)
        M, W, bc = physics(NC, r)
        M, W, bc = t64(M), t64(W), torch.as_tensor(bc)
        x64, ls64 = t64(x, True), t64(ls, True)
        uc = oelbo.rom_solve(M, torch.exp(x64) + 1e-8, t64(F), bc)
        mu = torch.einsum('sk,nk->ns', W, uc)
        Y = (mu.detach().numpy() + 0.3 * rng.normal(size=(N, dy))).astype(np.float32)
        Lo = oelbo.dgll(t64(Y), mu, 2 * ls64.repeat(N, 1))
        (-Lo).backward()
        _REF[key] = dict(x=x, F=F, ls=ls, Y=Y, dy=dy, mu=mu.detach().numpy(), uc=uc.detach().numpy(), L=Lo.item(),
                         gx=x64.grad.numpy(), gls=ls64.grad.numpy())
    return _REF[key]


def rom_desc(r, n, mode, **kw):
    """gpi_rom through its descriptor (every field reachable, unlike gpi.engine.rom_call)."""
    from gpi import _lib as L
    d = L.RomDesc()
    d.nc, d.refine, d.n, d.mode = NC, r, n, mode
    keep = []
    for k, v in kw.items():
        if torch.is_tensor(v):
            keep.append(v)
            v = v.data_ptr()
        setattr(d, k, v)
    L.check(L.lib().gpi_rom(C.byref(d), L.stream_handle()), 'rom')
    torch.cuda.synchronize()


def loglik(c, r, N, part=False, **kw):
    """One LOGLIK launch on case c -> (gx, d/dlogsigma_y [dy] fp64 or rows [N, dy], loss_acc, flag, uc, mu)."""
    from gpi import _lib as L
    x, F, Y, ls = cuda(c['x']), cuda(c['F']), cuda(c['Y']), cuda(c['ls'])
    gx = torch.zeros_like(x)
    acc = torch.zeros(L.GPI_REPLICAS, dtype=torch.float64, device='cuda')
    flag = torch.zeros(1, dtype=torch.int32, device='cuda')
    uc = torch.empty(N, NN, device='cuda')
    mu = torch.empty(N, c['dy'], device='cuda')
    if part:
        g = torch.full((N, c['dy']), float('nan'), device='cuda')
        kw['gls_part'] = g
    else:
        g = torch.zeros(c['dy'], dtype=torch.float64, device='cuda')
        kw['gacc_logsig'] = g
    rom_desc(r, N, L.ROM_LOGLIK, x=x, x_stride=NT2, F=F, Y=Y, logsig_y=ls, gx=gx, gx_stride=NT2, loss_acc=acc,
             flag=flag, uc=uc, mu_y=mu, loss_scale=1.0, **kw)
    return gx, g, acc, flag, uc, mu


# ---------------------------------------------------------------- 1. operator forward + backward
@pytest.mark.parametrize('r,N', [(1, 8), (2, 8), (8, 2)])
def test_rom16_operator(device, r, N):
    """RomOperatorFunction.apply (FORWARD with mu_y and uc, then BACKWARD with dmu) vs oelbo.rom_operator in fp64."""
    from gpi.native import RomOperatorFunction
    c = ref_case(r, N, 100 + r)
    x = cuda(c['x']).requires_grad_(True)
    mu, uc = RomOperatorFunction.apply(x, cuda(c['F']), NC, r, False)
    e_mu, e_uc = tensor_rel(mu.detach().cpu(), c['mu']), tensor_rel(uc.detach().cpu(), c['uc'])
    ls = cuda(c['ls']).requires_grad_(True)
    L = torch.sum(-0.5 * (2 * ls + (cuda(c['Y']) - mu) ** 2 * torch.exp(-2 * ls) + 1.8378770664093453))
    (-L).backward()
    e_L = abs(L.item() - c['L']) / abs(c['L'])
    e_gx, e_gls = tensor_rel(x.grad.cpu(), c['gx']), tensor_rel(ls.grad.cpu(), c['gls'])
    print('r %d N %d: mu %.2e uc %.2e L %.2e gx %.2e gls %.2e' % (r, N, e_mu, e_uc, e_L, e_gx, e_gls))
    assert e_mu < 1e-5 and e_uc < 1e-5
    assert e_L <= 1e-5
    assert e_gx < 1e-4
    assert e_gls < 1e-5


# ---------------------------------------------------------------- 2. fused LOGLIK
@pytest.mark.parametrize('r,N', [(2, 1), (1, 3), (2, 70), (8, 2)])
def test_rom16_fused_loglik(device, r, N):
    """gpi_rom LOGLIK (the ELBO engine's launch): value, gx and the gacc_logsig sum within the bars; the gls_part
    form finite everywhere, its sum within 1e-5, gx and loss_acc bit-identical to the atomic form; flag == 0."""
    c = ref_case(r, N, 200 + 10 * r + N)
    gx, gls, acc, flag, uc, mu = loglik(c, r, N)
    e_L = abs(acc.sum().item() - c['L']) / abs(c['L'])
    e_gx, e_gls = tensor_rel(gx.cpu(), c['gx']), tensor_rel(gls.cpu(), c['gls'])
    e_mu, e_uc = tensor_rel(mu.cpu(), c['mu']), tensor_rel(uc.cpu(), c['uc'])
    print('r %d N %d: L %.2e gx %.2e gls %.2e mu %.2e uc %.2e' % (r, N, e_L, e_gx, e_gls, e_mu, e_uc))
    assert e_L <= 1e-5
    assert e_gx < 1e-4
    assert e_gls < 1e-5
    assert e_mu < 1e-5 and e_uc < 1e-5
    assert flag.item() == 0
    gx2, part, acc2, flag2, _, _ = loglik(c, r, N, part=True)
    assert torch.isfinite(part).all()
    assert tensor_rel(part.double().sum(0).cpu(), c['gls']) < 1e-5
    assert torch.equal(gx2, gx) and torch.equal(acc2, acc)
    assert flag2.item() == 0


def test_rom16_loss_scale_and_replicas(device):
    """loss_scale multiplies gx and d/dlogsigma_y (not the value); sample s adds to loss_acc[s % GPI_REPLICAS]."""
    from gpi import _lib as L
    r, N = 1, 3
    c = ref_case(r, N, 200 + 10 * r + N)
    gx, gls, acc, _, _, _ = loglik(c, r, N)
    x, F, Y, ls = cuda(c['x']), cuda(c['F']), cuda(c['Y']), cuda(c['ls'])
    gx2 = torch.zeros_like(x)
    gls2 = torch.zeros_like(gls)
    acc2 = torch.zeros_like(acc)
    rom_desc(r, N, L.ROM_LOGLIK, x=x, x_stride=NT2, F=F, Y=Y, logsig_y=ls, gx=gx2, gx_stride=NT2, loss_acc=acc2,
             gacc_logsig=gls2, loss_scale=0.25)
    assert torch.equal(acc2, acc)
    assert tensor_rel(gx2.cpu(), 0.25 * c['gx']) < 1e-4
    assert tensor_rel(gls2.cpu(), 0.25 * c['gls']) < 1e-5
    assert int((acc != 0).sum().item()) == min(N, L.GPI_REPLICAS)


# ---------------------------------------------------------------- 3. BACKWARD
@pytest.mark.parametrize('which', ['dmu', 'duc', 'both'])
def test_rom16_backward(device, which):
    """BACKWARD with dmu only, duc only and both vs fp64 autograd of J = <dmu, mu> + <duc, u_c>."""
    from gpi import _lib as L
    r, N = 2, 8
    c = ref_case(r, N, 100 + r)
    rng = np.random.default_rng(31)
    dmu = rng.normal(size=(N, c['dy'])).astype(np.float32)
    duc = rng.normal(size=(N, NN)).astype(np.float32)
    M, W, bc = physics(NC, r)
    x64 = t64(c['x'], True)
    u = oelbo.rom_solve(t64(M), torch.exp(x64) + 1e-8, t64(c['F']), torch.as_tensor(bc))
    J = 0
    if which in ('dmu', 'both'):
        J = J + (t64(dmu) * torch.einsum('sk,nk->ns', t64(W), u)).sum()
    if which in ('duc', 'both'):
        J = J + (t64(duc) * u).sum()
    J.backward()
    x = cuda(c['x'])
    gx = torch.full_like(x, float('nan'))
    kw = {}
    if which in ('dmu', 'both'):
        kw['dmu'] = cuda(dmu)
    if which in ('duc', 'both'):
        kw['duc'] = cuda(duc)
    rom_desc(r, N, L.ROM_BACKWARD, x=x, x_stride=NT2, F=cuda(c['F']), gx=gx, gx_stride=NT2, **kw)
    e = tensor_rel(gx.cpu(), x64.grad.numpy())
    print(which, 'gx %.2e' % e)
    assert e < 1e-4


# ---------------------------------------------------------------- 4. options
def test_rom16_input_kappa(device):
    """input_kappa = 1: x holds kappa itself (ROM.__call__); gx is d/dkappa."""
    from gpi import _lib as L
    r, N = 1, 8
    c = ref_case(r, N, 100 + r)
    kap = (np.exp(c['x'].astype(np.float64)) + 1e-8).astype(np.float32)
    M, W, bc = physics(NC, r)
    k64 = t64(kap, True)
    u = oelbo.rom_solve(t64(M), k64, t64(c['F']), torch.as_tensor(bc))
    mu_o = torch.einsum('sk,nk->ns', t64(W), u)
    dmu = np.random.default_rng(5).normal(size=mu_o.shape).astype(np.float32)
    (t64(dmu) * mu_o).sum().backward()
    k, F = cuda(kap), cuda(c['F'])
    mu = torch.empty(N, c['dy'], device='cuda')
    uc = torch.empty(N, NN, device='cuda')
    rom_desc(r, N, L.ROM_FORWARD, input_kappa=1, x=k, x_stride=NT2, F=F, mu_y=mu, uc=uc)
    assert tensor_rel(mu.cpu(), mu_o.detach()) < 1e-5
    assert tensor_rel(uc.cpu(), u.detach()) < 1e-5
    gk = torch.empty_like(k)
    rom_desc(r, N, L.ROM_BACKWARD, input_kappa=1, x=k, x_stride=NT2, F=F, dmu=cuda(dmu), gx=gk, gx_stride=NT2)
    assert tensor_rel(gk.cpu(), k64.grad) < 1e-4


def test_rom16_x_draw_and_padded_accumulate(device):
    """x_draw: the q_X sample drawn in the kernel equals the stored-x launch on fmaf(expf(ls), eps, mu) bit for
    bit (rows at a padded x_stride).  gx_accumulate with a padded gx_stride adds into a pre-filled buffer and
    leaves the padding untouched."""
    r, N = 2, 3
    c = ref_case(r, N, 200 + 10 * r + N)
    rng = np.random.default_rng(8)
    xs = NT2 + 24
    mu_x = torch.zeros(N, xs, device='cuda')
    ls_x = torch.zeros(N, xs, device='cuda')
    eps = torch.zeros(N, xs, device='cuda')
    mu_x[:, :NT2] = cuda(c['x'])
    # log-sigmas 0 and -inf: expf is exact there (1 and 0) in every implementation, so the expected sample does
    # not depend on whose expf rounds how; both values show that x_ls is read
    ls_x[:, :NT2] = cuda(np.where(rng.random((N, NT2)) < 0.5, 0.0, -np.inf))
    eps[:, :NT2] = 0.05 * cuda(rng.normal(size=(N, NT2)))
    # fmaf in fp32: exact product and sum in fp64 (24-bit operands), rounded once
    xst = (torch.exp(ls_x).double() * eps.double() + mu_x.double()).float().contiguous()
    assert not torch.equal(xst, mu_x)
    c2 = dict(c)
    c2['x'] = xst[:, :NT2].cpu().numpy()
    gx0, g0, acc0, _, uc0, mu0 = loglik(c2, r, N, part=True)
    from gpi import _lib as L
    F, Y, ls = cuda(c['F']), cuda(c['Y']), cuda(c['ls'])
    gs = NT2 + 8
    pre = cuda(rng.normal(size=(N, gs)))
    gx1 = pre.clone()
    acc1 = torch.zeros_like(acc0)
    g1 = torch.full_like(g0, float('nan'))
    uc1, mu1 = torch.empty_like(uc0), torch.empty_like(mu0)
    rom_desc(r, N, L.ROM_LOGLIK, x_draw=1, x=mu_x, x_mu=mu_x, x_ls=ls_x, x_eps=eps, x_stride=xs, F=F, Y=Y,
             logsig_y=ls, gx=gx1, gx_stride=gs, gx_accumulate=1, loss_acc=acc1, gls_part=g1, uc=uc1, mu_y=mu1,
             loss_scale=1.0)
    assert torch.equal(uc1, uc0) and torch.equal(mu1, mu0) and torch.equal(g1, g0) and torch.equal(acc1, acc0)
    assert torch.equal(gx1[:, NT2:], pre[:, NT2:])
    # the kernel adds its last product into the buffer as one FMA (contraction), the stored form rounds the
    # product first: at most half an ulp of the term plus one rounding of the sum apart
    want = pre[:, :NT2].double() + gx0.double()
    bound = 2.0 ** -22 * (pre[:, :NT2].abs() + gx0.abs()).double()
    assert ((gx1[:, :NT2].double() - want).abs() <= bound).all()
    assert not torch.equal(gx1[:, :NT2], pre[:, :NT2])


def test_rom16_flag(device):
    """One input_kappa entry <= 1e-12 in one row raises the flag; the other rows of the launch keep their bits."""
    from gpi import _lib as L
    r, N = 1, 3
    c = ref_case(r, N, 200 + 10 * r + N)
    kap = (np.exp(c['x'].astype(np.float64)) + 1e-8).astype(np.float32)
    F = cuda(c['F'])
    out = []
    for poke in (False, True):
        k = cuda(kap)
        if poke:
            k[1, 77] = 1e-13
        flag = torch.zeros(1, dtype=torch.int32, device='cuda')
        mu = torch.empty(N, c['dy'], device='cuda')
        uc = torch.empty(N, NN, device='cuda')
        rom_desc(r, N, L.ROM_FORWARD, input_kappa=1, x=k, x_stride=NT2, F=F, mu_y=mu, uc=uc, flag=flag)
        uc2 = torch.empty(N, NN, device='cuda')
        flag2 = torch.zeros(1, dtype=torch.int32, device='cuda')
        rom_desc(r, N, L.ROM_FORWARD, input_kappa=1, x=k, x_stride=NT2, F=F, uc=uc2, flag=flag2)   # coarse-only form
        assert flag.item() == flag2.item() == int(poke)
        out.append((mu, uc, uc2))
    for a, b in zip(*out):
        assert torch.equal(a[[0, 2]], b[[0, 2]])


# ---------------------------------------------------------------- 5. per-sample independence
def test_rom16_rows_do_not_depend_on_batch_mates(device):
    """Rows of an N = 70 launch have the same bits in uc, mu_y, gx and gls_part as the N = 1 launch of the row."""
    r, N = 2, 70
    c = ref_case(r, N, 200 + 10 * r + N)
    gx, part, _, _, uc, mu = loglik(c, r, N, part=True)
    for i in (0, 33, 69):
        ci = dict(c)
        for k in ('x', 'F', 'Y'):
            ci[k] = c[k][i:i + 1]
        gxi, parti, _, _, uci, mui = loglik(ci, r, 1, part=True)
        assert torch.equal(uci[0], uc[i]) and torch.equal(mui[0], mu[i])
        assert torch.equal(gxi[0], gx[i]) and torch.equal(parti[0], part[i])


# ---------------------------------------------------------------- 6. coarse-only forward
@pytest.mark.parametrize('N', [200, 1])
def test_rom16_coarse_only_forward(device, N):
    """FORWARD with uc and without mu_y (one wave per sample, two per workgroup; N = 1 and the even N = 200 leave a
    ragged and a full last workgroup): within 2e-6 of the full forward's uc, four rows within 1e-5 of fp64."""
    from gpi import _lib as L
    r = 2
    _, x, F, _, dy = inputs(r, N, 600 + N)
    xd, Fd = cuda(x), cuda(F)
    uc = torch.full((N + 1, NN), float('nan'), device='cuda')
    rom_desc(r, N, L.ROM_FORWARD, x=xd, x_stride=NT2, F=Fd, uc=uc)
    assert torch.isnan(uc[N]).all()                       # the row past the batch is not written
    uc = uc[:N]
    uc_full = torch.empty(N, NN, device='cuda')
    mu = torch.empty(N, dy, device='cuda')
    rom_desc(r, N, L.ROM_FORWARD, x=xd, x_stride=NT2, F=Fd, uc=uc_full, mu_y=mu)
    assert tensor_rel(uc.cpu(), uc_full.cpu().numpy().astype(np.float64)) < 2e-6
    sel = sorted({0, N // 3, N // 2, N - 1})
    M, _, bc = physics(NC, r)
    u = oelbo.rom_solve(t64(M), torch.exp(t64(x[sel])) + 1e-8, t64(F[sel]), torch.as_tensor(bc))
    assert tensor_rel(uc[sel].cpu(), u) < 1e-5


# ---------------------------------------------------------------- 7. new vs generic kernel
CHILD = r'''
import sys
sys.path[:0] = [%r, %r, %r]
import numpy as np, torch
import test_gpu_rom16 as T
c = T.ref_case(2, 8, 102)
gx, gls, acc, flag, uc, mu = T.loglik(c, 2, 8)
np.savez(sys.argv[1], gx=gx.cpu().numpy(), gls=gls.cpu().numpy(), L=acc.sum().item(), uc=uc.cpu().numpy(),
         mu=mu.cpu().numpy(), flag=flag.item())
''' % (TESTS, ROOT, PKG)


def test_rom16_native_vs_generic_kernel(device, tmp_path):
    """LOGLIK at r = 2, N = 8 by the nc = 16 kernels and by the generic barrier-per-step kernel (GPI_ROM_SLOW=1, read
    once per process: one child process per arm): each arm within the bars of fp64, the arms within 2e-5 (mu) and
    2e-4 (gx) of each other."""
    c = ref_case(2, 8, 102)
    res = {}
    for name, slow in (('native', None), ('generic', '1')):
        env = {k: v for k, v in os.environ.items() if k != 'GPI_ROM_SLOW'}
        if slow:
            env['GPI_ROM_SLOW'] = slow
        path = str(tmp_path / (name + '.npz'))
        r = subprocess.run([sys.executable, '-c', CHILD, path], env=env, capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, (name, r.stdout[-2000:], r.stderr[-3000:])
        a = res[name] = np.load(path)
        errs = dict(mu=tensor_rel(a['mu'], c['mu']), uc=tensor_rel(a['uc'], c['uc']),
                    L=abs(float(a['L']) - c['L']) / abs(c['L']), gx=tensor_rel(a['gx'], c['gx']),
                    gls=tensor_rel(a['gls'], c['gls']))
        print(name, errs)
        assert errs['mu'] < 1e-5 and errs['uc'] < 1e-5 and errs['L'] <= 1e-5 and errs['gls'] < 1e-5
        assert errs['gx'] < 1e-4
        assert int(a['flag']) == 0
    assert tensor_rel(res['native']['mu'], res['generic']['mu']) < 2e-5
    assert tensor_rel(res['native']['gx'], res['generic']['gx']) < 2e-4
    # the two arms are different kernels: some bit differs
    assert not np.array_equal(res['native']['gx'], res['generic']['gx'])


# ---------------------------------------------------------------- 8. / 9. the ELBO and the fused step
class _DS(object):
    def __init__(self, perm=None, **t):
        self.t = t
        self.perm = perm
        self.N = next(iter(t.values())).shape[0]

    def __bool__(self):
        return True

    def get(self, key, random_subset=None):
        if random_subset is None:
            return self.t[key]
        return self.t[key][self.perm[:random_subset]]


def check_mask_audit(max_abs=1e-4, max_frac=1e-5):
    """The decisions taken from the kernels differ from the oracle's own sign tests only at ties (test_gpu_c64)."""
    n_dis = sum(a[1] for a in ocodec.MASK_AUDIT)
    n_all = sum(a[3] for a in ocodec.MASK_AUDIT)
    worst = max((a[2] for a in ocodec.MASK_AUDIT), default=0.0)
    rep = [a for a in ocodec.MASK_AUDIT if a[1]]
    assert n_all > 0
    assert worst < max_abs, rep
    assert n_dis <= max_frac * n_all, rep
    ocodec.MASK_AUDIT.clear()


def rom16_model(ident, over, n, Nu, Ns, seed):
    """A factory model with a 16 x 16 coarse mesh, random-init parameters and synthetic data (as
    test_fused_step_scaleup_grids builds them) -> (model, numpy data)."""
    from factories.model import ModelFactory
    torch.manual_seed(seed)
    fac = ModelFactory.FromIdentifier(ident)
    fac.set('device', 'cuda')
    fac.set(over)
    physics_, model, _, encoder, _, _ = fac.setup()
    model.encoder = encoder.cuda()
    assert physics_['rom'].grid.n == NC and physics_['fom'].grid.n == n
    assert model.g.dim_effective_property == NT2
    rng = np.random.default_rng(n)
    Xu = rng.normal(0.3, 0.6, (Nu, n, n)).astype(np.float32)
    Xs = rng.normal(0.3, 0.6, (Ns, n, n)).astype(np.float32)
    Y = rng.normal(0.0, 0.3, (Ns, (n + 1) * (n - 1))).astype(np.float32)
    F = np.zeros((Ns, NN), dtype=np.float32)
    F[:, BNODES] = rng.uniform(-0.5, 0.5, (Ns, len(BNODES)))
    model.register_datasets({'supervised': _DS(X=cuda(Xs), Y=cuda(Y), F_ROM_BC=cuda(F)),
                             'unsupervised': _DS(perm=torch.arange(Nu, device='cuda'), X=cuda(Xu))}, None,
                            create_unsupervised_variational_approximation=False)
    model.cuda()
    return model, dict(Xu=Xu, Xs=Xs, Y=Y, F=F)


def step_vs_oracle(model, D, n, bs, Ns, module_path):
    """One FusedElboStep.forward_backward() (and, module_path, model.elbo + backward of a copy on the same subset,
    noise and dropout scales) vs oracle_elbo with the kernels' ReLU decisions: value 1e-5, every gradient tensor
    5e-5 (check_grads), mask audit.  Returns the step."""
    from gpu_masks import engine_relu_masks
    from gpi.train import FusedElboStep
    import copy
    ref_model = copy.deepcopy(model)
    step = FusedElboStep(model, cuda(D['Xu']), bs, cuda(D['Xs']), cuda(D['Y']), cuda(D['F']), lr=1e-3, seed=5)
    e = step.engine
    eps_z_t, eps_x_t = e.eps_z().clone(), e.eps_x().clone()
    drops_t = {k: {nm: v.clone() for nm, v in dd.items()} for k, dd in e.dropout_views().items()}
    idx_t = step.idx.clone().long()
    st = {k: torch.tensor(p.detach().cpu().numpy(), dtype=torch.float64, requires_grad=True)
          for k, p in model.named_parameters()}
    ref_model._datasets['unsupervised'].perm = idx_t
    ref = ref_model.elbo(step=0, armortized_bs=bs, eps=(eps_z_t, eps_x_t), dropout=drops_t or None)
    masks = engine_relu_masks(ref_model._elbo_engine(bs, Ns, False))
    step.forward_backward()
    torch.cuda.synchronize()
    eps_z = eps_z_t.cpu().numpy().astype(np.float64)
    eps_x = eps_x_t.cpu().numpy().astype(np.float64)
    idx = idx_t.cpu().numpy()
    drops = {k: {nm: v.double().cpu() for nm, v in dd.items()} for k, dd in drops_t.items()}
    ocodec.MASK_AUDIT.clear()
    val = oracle_elbo(st, D['Xu'][idx], D['Xs'], D['Y'], D['F'], eps_z[:bs], eps_z[bs:], eps_x, NC, n // NC, masks=masks,
                      drops=drops or None)
    check_mask_audit()
    (-val).backward()
    got = step.elbo().item()
    print('elbo fused %.8g module %.8g oracle %.8g' % (got, ref.item(), val.item()))
    assert abs(got - val.item()) <= 1e-5 * abs(val.item()), (got, val.item())
    assert abs(ref.item() - val.item()) <= 1e-5 * abs(val.item()), (ref.item(), val.item())
    G = step.flat.G
    off = step.flat.name_offsets
    errs = {k: tensor_rel(G[off[k]:off[k] + st[k].numel()].cpu().numpy().reshape(st[k].shape), st[k].grad.numpy())
            for k in st}
    print('fused step')
    print(check_grads(errs, tol_all=5e-5, frac_tight=1.0))
    if module_path:
        (-ref).backward()
        errs = {k: tensor_rel(p.grad.cpu().numpy(), st[k].grad.numpy()) for k, p in ref_model.named_parameters()}
        print('module path')
        print(check_grads(errs, tol_all=5e-5, frac_tight=1.0))
    return step


def test_rom16_elbo_32(device):
    """highres32's codec on a 16 x 16 coarse mesh (r = 2), B_u = 4 of 8, N_s = 3: model.elbo + backward and one
    FusedElboStep.forward_backward() vs the fp64 oracle."""
    model, D = rom16_model('highres32', {'nx_rom': 16, 'ny_rom': 16, 'num_refines': 1}, 32, 8, 3, 3)
    step_vs_oracle(model, D, 32, 4, 3, True)


def test_rom16_fused_step_128(device):
    """highres128_rom16 (128^2, r = 8), B_u = 4 of 8, N_s = 2: one fused step vs the fp64 oracle; then capture() and
    two replays leave what two eager steps of a twin leave, bit for bit."""
    import copy
    from gpi.train import FusedElboStep
    model, D = rom16_model('highres128_rom16', {}, 128, 8, 2, 3)
    twin_a, twin_b = copy.deepcopy(model), copy.deepcopy(model)
    step_vs_oracle(model, D, 128, 4, 2, False)
    args = (cuda(D['Xu']), 4, cuda(D['Xs']), cuda(D['Y']), cuda(D['F']))
    eager = FusedElboStep(twin_a, *args, lr=1e-3, seed=5)
    graph = FusedElboStep(twin_b, *args, lr=1e-3, seed=5)
    graph.capture()
    for _ in range(2):
        eager.step()
        graph.step()
    torch.cuda.synchronize()
    assert graph.step_ctr.item() == eager.step_ctr.item() == 2
    assert torch.equal(graph.elbo(), eager.elbo())
    assert torch.equal(graph.flat.P, eager.flat.P)


# ---------------------------------------------------------------- 10. users of the coarse-only path
def test_rom16_update_virtual_observables(device):
    """update_virtual_observables on the 32 x 32 / 16 x 16 model: N_vo = 4 VO samples with CGR rows, N_mc = 16
    injected draws -- 64 coarse-only solves, then gpi_vo_moments and the conditioning -- vs oracle_vo_updates:
    MC mean / std 1e-5 (the bar of test_gpu_vo)."""
    from elbo_ref import oracle_vo_updates
    from bottleneck import VirtualObservables as VO
    from physics.BoundaryConditions import BoundaryCondition
    from physics.grid import pixel_to_cells
    from factories.model import ModelFactory
    n, r, Nu, Ns, Nvo, Nmc = 32, 2, 8, 3, 4, 16
    torch.manual_seed(3)
    fac = ModelFactory.FromIdentifier('highres32', device='cuda', nx_rom=16, ny_rom=16, num_refines=1)
    physics_, model, _, encoder, _, _ = fac.setup()
    model.encoder = encoder.cuda()
    rng = np.random.default_rng(77)
    img = lambda k: rng.normal(0.3, 0.6, (k, n, n)).astype(np.float32)
    Xu, Xs, Xv = img(Nu), img(Ns), img(Nvo)
    dy = (n + 1) * (n - 1)
    rom_grid = physics_['rom'].grid
    force = lambda k: (lambda U: (U, np.stack([rom_grid.full_force(u) for u in U]).astype(np.float32)))(
        rng.uniform(-0.5, 0.5, (k, 4)))
    _, Fs = force(Ns)
    Uv, Fv = force(Nvo)
    Ys, Yv = (rng.normal(0.0, 0.3, (k, dy)).astype(np.float32) for k in (Ns, Nvo))
    phys = {'fom': physics_['fom'], 'rom': physics_['rom'], 'W': np.asarray(physics_['W'], dtype=np.float64)}
    QPE = VO.QuerryPointEnsemble([VO.QuerryPoint(phys['fom'], pixel_to_cells(x.astype(np.float64)), BoundaryCondition(u))
                                  for x, u in zip(Xv, Uv)])
    QE = VO.QuerryEnsemble.FromQuerryPointEnsemble(QPE, phys, True, False, 0, 0, dtype=torch.float32,
                                                   device=torch.device('cuda'))
    ens = VO.VirtualObservablesEnsemble(QPE, QE, dtype=torch.float32, device=torch.device('cuda'))
    model.register_datasets({'supervised': _DS(X=cuda(Xs), Y=cuda(Ys), F_ROM_BC=cuda(Fs)),
                             'unsupervised': _DS(perm=torch.arange(Nu, device='cuda'), X=cuda(Xu)),
                             'vo': _DS(X=cuda(Xv), Y=cuda(Yv), F_ROM_BC=cuda(Fv))}, ens,
                            create_unsupervised_variational_approximation=False)
    model.cuda()
    with torch.no_grad():       # a q_X['vo'] away from its initial state
        model.q_X['vo']._mean.copy_(cuda(rng.normal(0.3, 0.7, (Nvo, NT2))))
        model.q_X['vo']._logsigma.copy_(cuda(rng.normal(-2.0, 0.3, (Nvo, NT2))))
    eps_X = rng.normal(size=(Nvo * Nmc, NT2)).astype(np.float32)
    eps_y = rng.normal(size=(Nvo * Nmc, dy)).astype(np.float32)
    Ym, Ysd = model.update_virtual_observables(Nmc, return_mean_stddev=True, step=0, eps=(cuda(eps_X), cuda(eps_y)))
    ens.check_flag()
    M, W, bc = physics(NC, r)
    d = {'state.' + k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
    d.update(cfg=np.array([n, NC, model.dim_latent, Nu, 4, Ns, Nvo, Nmc]), M=M, W=W, bc_dofs=np.asarray(bc),
             Gamma=QE.gamma.cpu().numpy(), alpha=QE.alpha.cpu().numpy(), Fv=Fv)
    d['upd0.eps_X'], d['upd0.eps_y'] = eps_X, eps_y
    assert d['Gamma'].shape[1] == NN            # the CGR rows, one per coarse node
    ups, _ = oracle_vo_updates(d, n_updates=1)
    e_m, e_s = tensor_rel(Ym.cpu(), ups[0]['Y_mean']), tensor_rel(Ysd.cpu(), ups[0]['Y_std'])
    e_post = tensor_rel(ens.mean.cpu(), ups[0]['mean'])
    print('VO update at nc = 16: MC mean %.2e std %.2e, posterior mean %.2e' % (e_m, e_s, e_post))
    assert e_m < 1e-5 and e_s < 1e-5


def test_rom16_surrogate_predictor(device):
    """SurrogatePredictor.predict at B = 3 on the 32 x 32 / 16 x 16 model (eval encoder -> gp mean -> gpi_rom
    FORWARD at nc = 16) vs its fp64 restatement, 1e-5."""
    import eval_ref
    from gpi.infer import SurrogatePredictor
    model, D = rom16_model('highres32', {'nx_rom': 16, 'ny_rom': 16, 'num_refines': 1}, 32, 8, 3, 3)
    gen = torch.Generator().manual_seed(17)
    st = model.encoder.state_dict()
    for k, v in st.items():
        if k.endswith('running_mean'):
            st[k] = (0.5 * torch.randn(v.shape, generator=gen)).cuda()
        elif k.endswith('running_var'):
            st[k] = (0.5 + torch.rand(v.shape, generator=gen)).cuda()
    model.encoder.load_state_dict(st)
    model.encoder.eval()
    p = SurrogatePredictor(model, 3)
    y = p.predict(cuda(D['Xs']), cuda(D['F'])).clone()
    p.check_flag()
    es = eval_ref.state64(dict(model.encoder.state_dict()), '')
    mu, _ = eval_ref.encoder_eval(es, D['Xs'], 32, [1, 1], 4, 4)
    w, b = model.gp.fc.weight.detach().double().cpu(), model.gp.fc.bias.detach().double().cpu()
    M, W, bc = physics(NC, 2)
    want, _ = oelbo.rom_operator(t64(W), t64(M), torch.as_tensor(bc), torch.as_tensor(mu) @ w.t() + b, t64(D['F']),
                                 model.g.logsigmas_y.detach().double().cpu())
    e = tensor_rel(y.cpu(), want.numpy())
    print('SurrogatePredictor.predict at nc = 16 vs fp64: %.2e' % e)
    assert y.shape == (3, 1023)
    assert e < 1e-5
