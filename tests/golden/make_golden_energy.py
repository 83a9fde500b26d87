"""Golden fixture of the energy virtual observables, from the REFERENCE's own classes.

Run where the reference checkout exists (see make_golden.py, whose helpers and module mocks this
imports), never on the GPU box:

    python tests/golden/make_golden_energy.py

vo_energy_elbo_c32.npz: the reference's EnergyVirtualObservablesEnsemble (VirtualObservables.py:1001-1037)
over the oracle's K_ff / f_eff at the c32 model of make_vo_elbo, exponential temperature schedule
(T_init 1, T_final 0.05, 4 steps), 3 inner iterations over 4 RBF test functions whose centres are recorded;
GenerativeModel.update_virtual_observables twice, then elbo (armortized + supervised + VO) and backward
with queued noise.  The stub sampler's sample_V() returns the RBF columns of the recorded centres in the
order the reference asks for them (per update: VO sample, then inner iteration).
"""
import os
from unittest import mock

import numpy as np
import torch

import make_golden as G
from make_golden import fem, random_fields, R_VO, R_ROM, R_comp, R_gen, CNNEncoder, CNNDecoder

HERE = os.path.dirname(os.path.abspath(__file__))
N_ITER, M_AUX, LENGTH = 3, 4, 0.15
SCHEDULE = dict(T_init=1.0, T_final=0.05, num_steps=4)


class _RecordedRBF(object):
    """sample_V() of the reference's RadialBasisFunctionSampler with the centres taken from a queue."""

    def __init__(self, P, length):
        self.P, self.length, self.queue = P, length, []

    def sample_V(self):
        c = self.queue.pop(0)
        return np.exp(-((self.P[:, 0:1] - c[None, :, 0]) ** 2 + (self.P[:, 1:2] - c[None, :, 1]) ** 2)
                      / self.length ** 2)


def _energy_ensemble(QPE, sampler):
    VO = R_VO.EnergyVirtualObservablesEnsemble(QPE, N_ITER, sampler, dtype=torch.float32, device=torch.device('cpu'))
    VO.set_temperature_schedule('exponential', **SCHEDULE)
    return VO


def _queue(sampler, centers):
    """centers [n_iter, N, m_aux, 2] in the reference's call order: VO sample, then inner iteration."""
    for n in range(centers.shape[1]):
        for it in range(centers.shape[0]):
            sampler.queue.append(centers[it, n])


def make_vo_energy_elbo():
    nc, r, mc, mf, M, W, cdofs, fdofs = G.c32_physics()
    n = nc * r
    rng = np.random.default_rng(18)
    Nu, bs, Ns, Nvo, Nmc = 8, 4, 3, 3, 6
    dz = 16
    torch.manual_seed(0)
    gen = torch.Generator().manual_seed(9)
    enc = CNNEncoder(n, dz, [1, 1], 4, 4, drop_rate=0)
    dec = CNNDecoder(n, dz, (8, 8), 1, 4, [1, 1], False, 4, drop_rate=0., upsample='nearest',
                     force_single_output=False, homoscedastic=False)
    G.randomize_bn(enc, gen)
    G.randomize_bn(dec, gen)
    rom = R_ROM.ROM(G._Phys(cdofs, fdofs), torch.tensor(M, dtype=torch.float32), torch.float32, 'cpu')
    g = R_comp.ReducedOrderModelOperator(rom, torch.tensor(W, dtype=torch.float32), dtype=torch.float32,
                                         device='cpu')
    gp = R_comp.EffectivePropertyMap(dz, M.shape[2], num_hidden_layers=0, independent_X=True,
                                     dtype=torch.float32, device='cpu')
    model = R_gen.GenerativeModel(f=dec, g=g, gp=gp, dtype=torch.float32, device='cpu')
    model.encoder = enc

    def labeled(k):
        img = random_fields(rng, k, n)
        U = rng.uniform(-0.5, 0.5, (k, 4))
        Y = np.stack([fem.solve_fom(mf, np.exp(fem.image_to_cells(x)), u) for x, u in zip(img, U)])
        F = np.stack([fem.f_rom_bc(mc, u) for u in U])
        return img, U, Y, F

    Xu = random_fields(rng, Nu, n)
    Xs, Us, Ys, Fs = labeled(Ns)
    Xv, Uv, Yv, Fv = labeled(Nvo)
    t32 = lambda a: torch.tensor(a, dtype=torch.float32)
    ds_sup = G._DS(X=t32(Xs), Y=t32(Ys), F_ROM_BC=t32(Fs))
    ds_uns = G._DS(X=t32(Xu))
    ds_vo = G._DS(X=t32(Xv), Y=t32(Yv), F_ROM_BC=t32(Fv))

    phys = G._FakePhysics(mf)
    QPs = [R_VO.QuerryPoint(phys, fem.image_to_cells(x), G._FakeBC(u)) for x, u in zip(Xv, Uv)]
    QPE = R_VO.QuerryPointEnsemble(QPs)
    P = mf.coords[fem.dirichlet_split(mf)[1]]
    sampler = _RecordedRBF(P, LENGTH)
    VO = _energy_ensemble(QPE, sampler)

    model.register_datasets({'supervised': ds_sup, 'unsupervised': ds_uns, 'vo': ds_vo}, VO,
                            create_unsupervised_variational_approximation=False)
    with torch.no_grad():
        for key in ('supervised', 'vo'):
            for q in (model.q_z[key], model.q_X[key]):
                q._mean.copy_(torch.tensor(rng.normal(0, 0.5, q._mean.shape)))
                q._logsigma.copy_(torch.tensor(rng.normal(-1.0, 0.3, q._logsigma.shape)))
        g.logsigmas_y.copy_(torch.tensor(rng.normal(-2.0, 0.2, g.logsigmas_y.shape)))
    state0 = {k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items()}
    dx = M.shape[2]
    dy = W.shape[0]

    class _Writer(object):
        def __init__(self):
            self.d = {}

        def add_scalar(self, k, v, global_step=None):
            self.d[k] = float(v)

    upd = []
    for it in range(2):
        centers = rng.uniform(0, 1, (N_ITER, Nvo, M_AUX, 2))
        _queue(sampler, centers)
        ex = rng.normal(size=(Nvo, Nmc, dx))
        ey = rng.normal(size=(Nvo, Nmc, dy))
        q_randn = [torch.tensor(e, dtype=torch.float32) for e in ex]
        q_like = [torch.tensor(e, dtype=torch.float32) for e in ey]

        def fake_randn(*size, **k):
            e = q_randn.pop(0)
            assert tuple(e.shape) == tuple(size), (e.shape, size)
            return e

        def fake_randn_like(t, *a, **k):
            e = q_like.pop(0)
            assert e.shape == t.shape
            return e

        model.writer = _Writer()
        with mock.patch('torch.randn', fake_randn), mock.patch('torch.randn_like', fake_randn_like):
            Ym, Ysd = model.update_virtual_observables(Nmc, return_mean_stddev=True, step=it)
        assert not q_randn and not q_like and not sampler.queue
        upd.append(dict(eps_X=ex.reshape(Nvo * Nmc, dx), eps_y=ey.reshape(Nvo * Nmc, dy), Y_mean=Ym.numpy(),
                        Y_std=Ysd.numpy(), mean=VO.mean.numpy(), vars=VO.vars.numpy(), centers=centers,
                        mean64=np.stack([vo._mean_np for vo in VO]), vars64=np.stack([vo._vars_np for vo in VO]),
                        temperature=np.float64(model.writer.d['Monitoring/Temperature'])))
        model.writer = None

    # conditioning of the fixture for the fp32 upstream: the same two updates on a fresh ensemble with Y_mean
    # perturbed by 1e-6 relative must move the posterior mean by less than 1e-5 relative
    s2 = _RecordedRBF(P, LENGTH)
    VO2 = _energy_ensemble(QPE, s2)
    for it, u in enumerate(upd):
        _queue(s2, u['centers'])
        Ym = torch.tensor(u['Y_mean'])
        Ym = Ym + 1e-6 * Ym.abs().max() * torch.tensor(rng.choice([-1.0, 1.0], Ym.shape), dtype=torch.float32)
        VO2.update(Ym, 1 / torch.tensor(u['Y_std']) ** 2, it)
        m2 = np.stack([vo._mean_np for vo in VO2])
        moved = np.abs(m2 - u['mean64']).max() / np.abs(u['mean64']).max()
        print('update %d: T %.4f, Y_mean + 1e-6 moves the posterior mean by %.2e' % (it, u['temperature'], moved))
        assert moved < 1e-5, moved

    perm = torch.tensor(rng.permutation(Nu), dtype=torch.long)
    shapes = [(bs, dz), (Ns, dz), (Ns, dx), (Nvo, dz), (Nvo, dx), (Nvo, dy)]
    eps = [torch.tensor(rng.normal(size=sh), dtype=torch.float32) for sh in shapes]
    queue = list(eps)

    def fake_randn_like(t, *a, **k):
        e = queue.pop(0)
        assert e.shape == t.shape, (e.shape, t.shape)
        return e.to(dtype=t.dtype)

    model.writer = _Writer()
    with mock.patch('torch.randperm', lambda N, **k: perm.clone()), mock.patch('torch.randn_like', fake_randn_like):
        elbo = model.elbo(step=0, armortized_bs=bs)
    assert not queue
    terms_main = dict(model.writer.d)
    model.writer = None
    (-elbo).backward()
    out = {'state.' + k: v for k, v in state0.items()}
    out.update({'grad.' + k: p.grad.detach().numpy().copy() for k, p in model.named_parameters()
                if p.grad is not None})
    out.update(Xu=Xu.astype(np.float32), Xs=Xs.astype(np.float32), Ys=Ys.astype(np.float32),
               Fs=Fs.astype(np.float32), Us=Us, Xv=Xv.astype(np.float32), Yv=Yv.astype(np.float32),
               Fv=Fv.astype(np.float32), Uv=Uv, Xv_dg=np.stack([qp.x for qp in QPs]), perm=perm.numpy(),
               M=M.astype(np.float32), W=W.astype(np.float32), bc_dofs=cdofs,
               cfg=np.array([n, nc, dz, Nu, bs, Ns, Nvo, Nmc]),
               energy_cfg=np.array([N_ITER, M_AUX, LENGTH, SCHEDULE['T_init'], SCHEDULE['T_final'],
                                    SCHEDULE['num_steps']]),
               elbo=np.float64(elbo.item()))
    for k, v in terms_main.items():
        out['term.' + k] = np.float64(v)
    for i, e in enumerate(eps):
        out['eps%d' % i] = e.numpy()
    for it, u in enumerate(upd):
        for k, v in u.items():
            out['upd%d.%s' % (it, k)] = v
    path = os.path.join(HERE, 'vo_energy_elbo_c32.npz')
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 1 << 20, os.path.getsize(path)
    print('vo energy elbo ok', elbo.item(), os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    make_vo_energy_elbo()
