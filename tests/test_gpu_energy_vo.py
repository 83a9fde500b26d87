"""Energy virtual observables on the GPU (gpi_vo_energy, csrc/energy.hip; bottleneck/VirtualObservables.py
EnergyVirtualObservablesEnsemble) against an fp64 numpy restatement of the reference's update
(VirtualObservables.py:769-788) over the oracle's assembled K_ff / f_eff, both kernel forms forced.

The fp64 bar is the project's (test_gpu_fom.py): max|x - ref| / max|ref| <= 1e-9.  The restatement in fp64
and in extended precision differ by <= 1.5e-14 at these inputs (cond(V^T A V) <= 1e4 is asserted on the
inputs of every iteration), so the bar has five orders of margin and passing it still proves every term.
The fp32 mirrors are compared for equality: mean32 = (float) mean, and logsig32 = 0.5 log((float) vars) with the
log taken in fp64 and rounded once, as the kernel documents it (a float log is only defined to an ulp, and the
device library's and torch's differ in that ulp)."""
import functools
import os

import numpy as np
import pytest
import torch

from oracle import fem

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
TOL = 1e-9
COND_MAX = 1e4


def cuda(a, dtype=torch.float64):
    return torch.tensor(np.asarray(a), dtype=dtype, device='cuda').contiguous()


def rel(a, b):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = np.asarray(b)
    return float(np.abs(a - b).max() / np.abs(b).max())


# ---------------------------------------------------------------- the restatement
@functools.lru_cache(maxsize=None)
def grid_case(nc, r, N=3, seed=0):
    """Inputs of one grid, assembled once: x ~ N(0.3, 0.9) per DG0 cell, u ~ U(-0.5, 0.5), K_ff / f_eff per
    sample (dense fp64), the free nodes' coordinates, and two (g, prec) sets (prec = 1 / sigma^2,
    sigma ~ U(0.01, 0.1)) for two consecutive updates."""
    rng = np.random.default_rng(100 + 10 * nc + r + seed)
    n = nc * r
    mf = fem.unit_square_mesh(n)
    P = mf.coords[fem.dirichlet_split(mf)[1]]
    dy = P.shape[0]
    assert dy == (n + 1) * (n - 1)
    x = rng.normal(0.3, 0.9, (N, 2 * n * n))
    u = rng.uniform(-0.5, 0.5, (N, 4))
    K, f = [], []
    for i in range(N):
        Ki, fi = fem.assemble_system(mf, np.exp(x[i]), u[i])
        K.append(np.asarray(Ki.todense()) if hasattr(Ki, 'todense') else np.asarray(Ki))
        f.append(np.asarray(fi).reshape(-1))
    g = rng.normal(0.0, 0.3, (2, N, dy)).astype(np.float32)
    prec = (1.0 / rng.uniform(0.01, 0.1, (2, N, dy)) ** 2).astype(np.float32)
    return dict(n=n, N=N, dy=dy, P=P, x=x, u=u, K=K, f=f, g=g, prec=prec)


def lattice_centers(rng, n_iter, N, m_aux):
    """m_aux <= 4: a jittered 2 x 2 lattice (l = 0.15); m_aux = 32: a jittered subset of a 6 x 6 lattice
    (l = 0.08).  Returns (centres [n_iter, N, m_aux, 2], l)."""
    if m_aux <= 4:
        base = np.array([[0.25, 0.25], [0.75, 0.25], [0.25, 0.75], [0.75, 0.75]])
        c = base[None, None, :m_aux] + rng.uniform(-0.1, 0.1, (n_iter, N, m_aux, 2))
        return c, 0.15
    k = (np.arange(6) + 0.5) / 6
    base = np.stack(np.meshgrid(k, k, indexing='ij'), -1).reshape(36, 2)
    c = np.empty((n_iter, N, m_aux, 2))
    for it in range(n_iter):
        for s in range(N):
            c[it, s] = base[rng.choice(36, m_aux, replace=False)] + rng.uniform(-0.02, 0.02, (m_aux, 2))
    return c, 0.08


def restate(K, f, P, g, prec, T, mean, centers, l):
    """One update of one sample: (mean, vars, [cond(V^T A V) per iteration]); fp64 numpy, dense, exactly
    the formulas of the reference (A = diag(prec) + K / T, b = f / T + prec * g)."""
    beta = 1.0 / T
    prec = prec.astype(np.float64)
    g = g.astype(np.float64)
    vars_ = 1.0 / (prec + beta * np.diag(K))
    A = np.diag(prec) + beta * K
    b = beta * f + prec * g
    conds = []
    mean = mean.copy()
    for c in centers:
        V = np.exp(-((P[:, 0:1] - c[None, :, 0]) ** 2 + (P[:, 1:2] - c[None, :, 1]) ** 2) / l ** 2)
        M = V.T @ A @ V
        conds.append(np.linalg.cond(M))
        mean = mean - V @ np.linalg.solve(M, V.T @ (A @ mean - b))
    return mean, vars_, conds


def restate_batch(case, upd, T, mean, centers, l, skip=()):
    out_m, out_v, conds = [], [], []
    for s in range(case['N']):
        if s in skip:
            m, v, _ = restate(case['K'][s], case['f'][s], case['P'], case['g'][upd, s], case['prec'][upd, s], T,
                              mean[s], centers[:0, s], l)
        else:
            m, v, c = restate(case['K'][s], case['f'][s], case['P'], case['g'][upd, s], case['prec'][upd, s], T,
                              mean[s], centers[:, s], l)
            conds += c
        out_m.append(m)
        out_v.append(v)
    return np.stack(out_m), np.stack(out_v), conds


def launch(case, upd, T, mean, m_aux, n_iter, l, form, centers=None, **kw):
    """gpi_vo_energy on update `upd`'s (g, prec); mean (device fp64) in/out.  Returns (vars, mean32, logsig32, flag)."""
    from gpi.vo import vo_energy
    N, dy = case['N'], case['dy']
    vars_ = torch.full((N, dy), -7.0, dtype=torch.float64, device='cuda')
    m32 = torch.full((N, dy), -7.0, dtype=torch.float32, device='cuda')
    l32 = torch.full((N, dy), -7.0, dtype=torch.float32, device='cuda')
    flag = torch.zeros(1, dtype=torch.int32, device='cuda')
    vo_energy(cuda(case['x']), cuda(case['u']), case['n'], cuda(case['g'][upd], torch.float32),
              cuda(case['prec'][upd], torch.float32), T, mean, vars_, m_aux, n_iter, l, mean32=m32, logsig32=l32,
              centers=cuda(centers) if centers is not None else None, flag=flag, form=form, **kw)
    return vars_, m32, l32, flag


def logsig_ref(vars_):
    """0.5 log((float) vars) rounded to fp32 once (the log in fp64), as the kernel documents it."""
    v32 = vars_.float().cpu().numpy()
    return torch.from_numpy((0.5 * np.log(v32.astype(np.float64))).astype(np.float32)).cuda()


def forms():
    from gpi import _lib as L
    return {'fused': L.VO_ENERGY_FUSED, 'tiled': L.VO_ENERGY_TILED}


# ---------------------------------------------------------------- 1. kernel vs the restatement
@pytest.mark.parametrize('form', ['fused', 'tiled'])
@pytest.mark.parametrize('n_iter', [1, 3])
@pytest.mark.parametrize('m_aux', [1, 4, 32])
@pytest.mark.parametrize('nc,r', [(2, 8), (3, 4), (4, 8)])
def test_energy_update_matches_restatement(device, nc, r, m_aux, n_iter, form):
    """Two consecutive updates (different g, prec and temperature: 1.0, then 0.05) on the persistent mean, injected
    centres; d_y = 255 (less than one 256-thread pass), 143 (12 x 12 squares, not a power of two), 1023."""
    case = grid_case(nc, r)
    rng = np.random.default_rng(7 + m_aux + 100 * n_iter)
    N, dy = case['N'], case['dy']
    mean = torch.zeros(N, dy, dtype=torch.float64, device='cuda')
    ref = np.zeros((N, dy))
    for upd, T in enumerate((1.0, 0.05)):
        cen, l = lattice_centers(rng, n_iter, N, m_aux)
        ref, ref_v, conds = restate_batch(case, upd, T, ref, cen, l)
        assert max(conds) <= COND_MAX, max(conds)                 # a condition on the inputs
        vars_, m32, l32, flag = launch(case, upd, T, mean, m_aux, n_iter, l, forms()[form], centers=cen)
        em, ev = rel(mean, ref), rel(vars_, ref_v)
        print('update %d T %.2f cond %.3g: mean %.2e vars %.2e' % (upd, T, max(conds), em, ev))
        assert em <= TOL and ev <= TOL, (upd, em, ev)
        assert torch.equal(m32, mean.float())
        assert torch.equal(l32, logsig_ref(vars_))
        assert int(flag.item()) == 0


@pytest.mark.parametrize('form', ['fused', 'tiled'])
def test_energy_zero_iterations_leaves_the_mean(device, form):
    case = grid_case(3, 4)
    rng = np.random.default_rng(3)
    start = rng.normal(size=(case['N'], case['dy']))
    mean = cuda(start)
    vars_, m32, l32, flag = launch(case, 0, 0.5, mean, 4, 0, 0.15, forms()[form])
    assert torch.equal(mean, cuda(start))
    _, ref_v, _ = restate_batch(case, 0, 0.5, start, np.zeros((0, case['N'], 4, 2)), 0.15)
    assert rel(vars_, ref_v) <= TOL
    assert torch.equal(m32, mean.float()) and torch.equal(l32, logsig_ref(vars_))


# ---------------------------------------------------------------- 2. device draws
def test_energy_device_draws(device):
    from gpi.vo import ENERGY_SUB
    from philox_ref import philox
    case = grid_case(2, 8)
    N, dy, m_aux, n_iter, l = case['N'], case['dy'], 4, 3, 0.15
    F = forms()

    def run(seed, form, offset=None):
        mean = torch.zeros(N, dy, dtype=torch.float64, device='cuda')
        cen = torch.full((n_iter, N, m_aux, 2), -1.0, dtype=torch.float64, device='cuda')
        out = launch(case, 0, 0.3, mean, m_aux, n_iter, l, form, seed=seed, centers_out=cen,
                     offset=torch.tensor([offset], dtype=torch.int64, device='cuda') if offset is not None else None)
        return mean, cen, out

    mean, cen, (vars_, m32, _, flag) = run(1234, F['fused'])
    c = cen.cpu().numpy()
    q = philox(np.arange(n_iter * N * m_aux, dtype=np.uint64), ENERGY_SUB, 1234)
    want = np.stack([q[0].astype(np.float64) * 2.0 ** -32, q[1].astype(np.float64) * 2.0 ** -32], -1)
    assert np.array_equal(c.reshape(-1, 2), want)                       # bit for bit, documented counters
    assert c.min() >= 0.0 and c.max() < 1.0
    assert np.abs(c[:, 0] - c[:, 1]).min() > 0 and np.abs(c[0] - c[1]).min() > 0     # samples, iterations
    ref, ref_v, conds = restate_batch(case, 0, 0.3, np.zeros((N, dy)), c, l)
    print('device draws: cond %.3g mean %.2e' % (max(conds), rel(mean, ref)))
    assert max(conds) <= COND_MAX, max(conds)                           # a condition on this seed's draws
    assert rel(mean, ref) <= TOL and rel(vars_, ref_v) <= TOL
    mean2, cen2, _ = run(1234, F['fused'])                              # same seed: the same bits
    assert torch.equal(mean2, mean) and torch.equal(cen2, cen)
    mean_t, cen_t, _ = run(1234, F['tiled'])                            # the tiled form draws the same centres
    assert torch.equal(cen_t, cen) and rel(mean_t, ref) <= TOL
    mean_t2, _, _ = run(1234, F['tiled'])
    assert torch.equal(mean_t2, mean_t)
    _, cen3, _ = run(99, F['fused'])
    assert np.abs(cen3.cpu().numpy() - c).min() > 0                     # another seed: other centres
    _, cen4, _ = run(1234, F['fused'], offset=5)                        # *offset shifts the counters
    q = philox(5 + np.arange(n_iter * N * m_aux, dtype=np.uint64), ENERGY_SUB, 1234)
    assert np.array_equal(cen4.cpu().numpy().reshape(-1, 2)[:, 0], q[0].astype(np.float64) * 2.0 ** -32)


# ---------------------------------------------------------------- public classes
class _Writer(object):
    def __init__(self):
        self.d = []

    def add_scalar(self, k, v, global_step=None):
        self.d.append((k, float(v), global_step))


def make_ensemble(case, m_aux, n_iter, l, dtype=torch.float32):
    from bottleneck import VirtualObservables as VO
    from physics.LinearElliptic import LinearEllipticPhysics
    from physics.BoundaryConditions import BoundaryCondition
    phys = LinearEllipticPhysics('fom', 'NDP', case['n'])
    QPE = VO.QuerryPointEnsemble([VO.QuerryPoint(phys, x, BoundaryCondition(u)) for x, u in zip(case['x'], case['u'])])
    sampler = VO.RadialBasisFunctionSampler(QPE[0], l=l, N_aux=m_aux, device=torch.device('cuda'))
    return VO.EnergyVirtualObservablesEnsemble(QPE, n_iter, sampler, dtype=dtype, device=torch.device('cuda'))


# ---------------------------------------------------------------- 3. degenerate subspace
@pytest.mark.parametrize('form', ['fused', 'tiled'])
def test_energy_degenerate_subspace_is_skipped(device, form):
    """Two identical centres for sample 1 in every iteration: its V^T A V is singular, the sample keeps its mean
    (finite), the flag is set and check_flag() raises; the other samples match the restatement."""
    case = grid_case(2, 8)
    rng = np.random.default_rng(5)
    N, dy, m_aux, n_iter = case['N'], case['dy'], 4, 2
    cen, l = lattice_centers(rng, n_iter, N, m_aux)
    cen[:, 1, 3] = cen[:, 1, 0]
    start = rng.normal(0, 0.1, (N, dy))
    ens = make_ensemble(case, m_aux, n_iter, l)
    ens._state.form = forms()[form]
    ens._state.mean64.copy_(cuda(start))
    ens.force_temperature(0.2)
    ens.queue_centers(cuda(cen))
    ens.update(cuda(case['g'][0], torch.float32), cuda(case['prec'][0], torch.float32), 0)
    ref, ref_v, conds = restate_batch(case, 0, 0.2, start, cen, l, skip=(1,))
    assert max(conds) <= COND_MAX
    mean = ens.mean64
    assert torch.isfinite(mean).all()
    assert torch.equal(mean[1], cuda(start)[1])
    assert rel(mean[[0, 2]], ref[[0, 2]]) <= TOL and rel(ens.vars64, ref_v) <= TOL
    with pytest.raises(RuntimeError, match='singular'):
        ens.check_flag()


# ---------------------------------------------------------------- 5. public surface
def test_energy_ensemble_public_surface(device):
    from bottleneck import VirtualObservables as VO
    case = grid_case(2, 8)
    N, dy, m_aux, n_iter, l = case['N'], case['dy'], 4, 3, 0.15
    ens = make_ensemble(case, m_aux, n_iter, l)
    assert ens.N == N and ens.m == 1 and ens.dim_out == dy and len(ens) == N
    assert ens.mean is None and ens.vars is None and ens.logsigma is None
    assert ens[0].mean is None and ens[0].vars is None
    G, PREC = cuda(case['g'][0], torch.float32), cuda(case['prec'][0], torch.float32)
    with pytest.raises(RuntimeError):
        ens.update(G, PREC, 0)                       # neither a schedule nor a forced temperature
    assert ens.mean is None
    ens.set_temperature_schedule('exponential', T_init=1.0, T_final=0.05, num_steps=4)
    w = _Writer()
    ens.resample()                                   # no-op
    cen, _ = lattice_centers(np.random.default_rng(1), n_iter, N, m_aux)
    ens.queue_centers(cuda(cen))
    ens.update(G, PREC, 1, writer=w)
    assert len(w.d) == 1 and w.d[0][0] == 'Monitoring/Temperature' and w.d[0][2] == 1
    assert w.d[0][1] == pytest.approx(0.05 ** (1 / 3), rel=1e-14)
    assert ens.temperature == pytest.approx(0.05 ** (1 / 3)) and ens[2].temperature == ens.temperature
    ref, ref_v, _ = restate_batch(case, 0, 0.05 ** (1 / 3), np.zeros((N, dy)), cen, l)
    assert rel(ens.mean64, ref) <= TOL
    # dtype rules of VirtualObservablesEnsemble: fp32 mirrors for a float32 model
    assert ens.mean.dtype == torch.float32 and ens.logsigma.dtype == torch.float32 and ens.vars.dtype == torch.float32
    assert torch.equal(ens.mean, ens.mean64.float()) and torch.equal(ens.logsigma, logsig_ref(ens.vars64))
    assert rel(ens.vars, ref_v) < 1e-6
    for n, vo in enumerate(ens):                     # members: fp64 views of the ensemble's rows
        assert vo.m == 1 and vo.mean.dtype == torch.float64
        assert vo.mean.data_ptr() == ens.mean64[n].data_ptr() and vo.vars.data_ptr() == ens.vars64[n].data_ptr()
    assert 'Current temperature' in repr(ens[0])
    ens.force_temperature(0.5)                       # a forced value overrides the schedule
    ens.update(G, PREC, 99)                          # ... and the schedule's range check with it
    assert ens.temperature == 0.5 and ens[0].temperature == 0.5
    ens.check_flag()
    # second update drew its centres on the device and carried the mean over
    assert rel(ens.mean64, ref) > 1e-6
    with pytest.raises(NotImplementedError, match='RadialBasisFunctionSampler'):
        VO.EnergyVirtualObservablesEnsemble(ens._QuerryPointEnsemble, n_iter,
                                            VO.GaussianSketchingSampler(ens._QuerryPointEnsemble[0], 4),
                                            dtype=torch.float32, device=torch.device('cuda'))
    # a VO on its own: a batch of one
    vo = VO.EnergyVirtualObservable(ens._QuerryPointEnsemble[0], n_iter, stochastic_subspace=m_aux, l=l,
                                    dtype=torch.float32, device=torch.device('cuda'))
    assert vo.mean is None
    vo.force_temperature(0.5)
    with pytest.raises(RuntimeError):
        vo.update(G[0], PREC[0], 0)
    vo.update(G[0], PREC[0], 0, ForceUpdate=True)
    assert vo.mean.shape == (dy,) and torch.isfinite(vo.mean).all()
    assert rel(vo.vars, 1.0 / (case['prec'][0, 0].astype(np.float64) + 2.0 * np.diag(case['K'][0]))) <= TOL


# ---------------------------------------------------------------- 4. end to end against the reference's own run
def build_energy_vo_model(d):
    """The c32 model of test_gpu_vo.build_vo_model with the energy ensemble in place of the constrain one."""
    from test_gpu_vo import _DS, cuda as c32
    from bottleneck.Encoder import CNNEncoder
    from bottleneck.Decoder import CNNDecoder
    from bottleneck.components import EffectivePropertyMap, ReducedOrderModelOperator
    from bottleneck.ROM import ROM
    from bottleneck.generative import GenerativeModel
    from bottleneck import VirtualObservables as VO
    from physics.grid import StructuredGrid
    from physics.LinearElliptic import LinearEllipticPhysics
    from physics.BoundaryConditions import BoundaryCondition
    n, nc, dz, Nu, bs, Ns, Nvo, Nmc = [int(v) for v in d['cfg']]
    n_iter, m_aux, length, T_init, T_final, steps = [float(v) for v in d['energy_cfg']]
    dev = torch.device('cuda')
    enc = CNNEncoder(n, dz, [1, 1], 4, 4, drop_rate=0)
    dec = CNNDecoder(n, dz, (8, 8), 1, 4, [1, 1], False, 4, drop_rate=0.)
    rom = ROM(StructuredGrid(nc), n // nc)
    g = ReducedOrderModelOperator(rom, torch.tensor(d['W']), dtype=torch.float32, device='cuda')
    gp = EffectivePropertyMap(dz, 2 * nc * nc, independent_X=True, dtype=torch.float32, device='cuda')
    model = GenerativeModel(f=dec.cuda(), g=g, gp=gp, dtype=torch.float32, device=dev)
    model.encoder = enc.cuda()
    fom = LinearEllipticPhysics('fom', 'NDP', n)
    QPE = VO.QuerryPointEnsemble([VO.QuerryPoint(fom, x, BoundaryCondition(u)) for x, u in zip(d['Xv_dg'], d['Uv'])])
    sampler = VO.RadialBasisFunctionSampler(QPE[0], l=length, N_aux=int(m_aux), device=dev)
    ens = VO.EnergyVirtualObservablesEnsemble(QPE, int(n_iter), sampler, dtype=torch.float32, device=dev)
    ens.set_temperature_schedule('exponential', T_init=T_init, T_final=T_final, num_steps=int(steps))
    ds_s = _DS(X=c32(d['Xs']), Y=c32(d['Ys']), F_ROM_BC=c32(d['Fs']))
    ds_u = _DS(perm=torch.tensor(d['perm'], device='cuda'), X=c32(d['Xu']))
    ds_v = _DS(X=c32(d['Xv']), Y=c32(d['Yv']), F_ROM_BC=c32(d['Fv']))
    model.register_datasets({'supervised': ds_s, 'unsupervised': ds_u, 'vo': ds_v}, ens,
                            create_unsupervised_variational_approximation=False)
    model.load_state_dict({k[6:]: torch.tensor(v) for k, v in d.items() if k.startswith('state.')})
    model.cuda()
    return model, ens, bs


@pytest.mark.parametrize('form', ['fused', 'tiled'])
def test_energy_vo_update_and_elbo_match_reference(device, form):
    """update_virtual_observables x2 (exponential schedule 1 -> 0.05 over 4 steps, 3 iterations, 4 RBF test
    functions at the recorded centres) + elbo + backward through the unchanged GenerativeModel, vs the
    reference's own run (tests/golden/make_golden_energy.py) and the fp64 oracle, at the bars of
    test_gpu_vo._vo_model_parity: posterior mean / vars per update 1e-5, ELBO vs the fixture 2e-5, ELBO vs the
    oracle given the native posterior 1e-5, gradients 5e-5 per tensor with the kernels' ReLU masks."""
    from elbo_ref import oracle_vo_fixture_elbo, tensor_rel, check_grads
    from gpu_masks import engine_relu_masks
    from test_gpu_c64 import check_mask_audit
    from test_gpu_vo import cuda as c32
    from oracle import codec as ocodec
    d = dict(np.load(os.path.join(HERE, 'golden', 'vo_energy_elbo_c32.npz')))
    model, ens, bs = build_energy_vo_model(d)
    ens._state.form = forms()[form]
    w = _Writer()
    model.writer = w
    for it in range(2):
        ens.queue_centers(cuda(d['upd%d.centers' % it]))
        Ym, Ys = model.update_virtual_observables(int(d['cfg'][7]), return_mean_stddev=True, step=it,
                                                  eps=(c32(d['upd%d.eps_X' % it]), c32(d['upd%d.eps_y' % it])))
        errs = dict(Y_mean=tensor_rel(Ym.cpu(), d['upd%d.Y_mean' % it]), Y_std=tensor_rel(Ys.cpu(), d['upd%d.Y_std' % it]),
                    mean=tensor_rel(ens.mean.cpu(), d['upd%d.mean' % it]), vars=tensor_rel(ens.vars.cpu(), d['upd%d.vars' % it]),
                    mean64=tensor_rel(ens.mean64.cpu(), d['upd%d.mean64' % it]),
                    vars64=tensor_rel(ens.vars64.cpu(), d['upd%d.vars64' % it]))
        print('update', it, errs)
        assert max(errs.values()) < 1e-5, (it, errs)
        assert ens.temperature == pytest.approx(float(d['upd%d.temperature' % it]), rel=1e-14)
    temps = [v for k, v, s in w.d if k == 'Monitoring/Temperature']
    assert temps == pytest.approx([1.0, 0.05 ** (1 / 3)], rel=1e-14)
    model.writer = None
    ens.check_flag()
    vo_mean, vo_vars = ens.mean.cpu().numpy(), ens.vars.cpu().numpy()

    e = [c32(d['eps%d' % i]) for i in range(6)]
    eps = (torch.cat([e[0], e[1], e[3]]), torch.cat([e[2], e[4]]), e[5])
    elbo = model.elbo(step=0, armortized_bs=bs, eps=eps)
    Ns, Nvo = int(d['cfg'][5]), int(d['cfg'][6])
    engine = model._elbo_engine(bs, Ns, False, N_vo=Nvo, vo_holdoff=False)
    ref = float(d['elbo'])
    print('elbo', elbo.item(), 'fixture', ref)
    assert abs(elbo.item() - ref) / abs(ref) < 2e-5
    (-elbo).backward()
    masks = engine_relu_masks(engine)
    ocodec.MASK_AUDIT.clear()
    val_o, gr_o = oracle_vo_fixture_elbo(d, vo_mean, vo_vars, masks=masks, lockx=False)
    check_mask_audit()
    assert abs(elbo.item() - val_o) <= 1e-5 * abs(val_o), (elbo.item(), val_o)
    errs = {k: tensor_rel(p.grad.cpu(), gr_o[k]) for k, p in model.named_parameters()}
    print(check_grads(errs, tol_all=5e-5, frac_tight=1.0))
