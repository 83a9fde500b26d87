"""Partially observed labels, from the REFERENCE's own run (run where the reference exists, never on the
GPU box; the reference is imported the way make_golden.py imports it, FEniCS & co. mocked):

    python tests/golden/make_golden_partial.py

elbo_partial_c32.npz: the reference's GenerativeModel.elbo + backward at the highres32 shapes (32 x 32, ROM
4 x 4, armortised encoder, freeX, B_u = 8 of a pool of 16, N_s = 4, injected noise and permutation, as
make_golden.py's make_elbo) with the label hook  model.preprocess_y_fct = lambda y: y[..., idx]  for a seeded
idx of 128 of the 1023 fine free nodes (generative.py:49-56,473).  Contents: inputs, noise, state dict, idx, the
ELBO, the per-term scalars the reference logs ('term.objective/...') and every gradient.  M is not stored
(elbo_ref.physics(4, 8) is the same tensor); W is, the test models take it from the fixture.

romfit_partial_c32.npz: the reference's OptimizeEffectiveProperties (bottleneck/utils.py:250-282) on the labels
and right-hand sides of rom_c32.npz (the inputs of romfit_c32.npz) with a y_preprocessor that selects a regular
sensor grid -- every second fine free node in both directions -- and make_golden_romfit.py's iteration count
and learning rate.  Only the outputs and the index set are stored.
"""
import os
from unittest import mock

import numpy as np
import torch

from make_golden import (CNNEncoder, CNNDecoder, R_ROM, R_comp, R_gen, R_utils, randomize_bn, random_fields, HERE,
                         _Phys, _DS, c32_physics, fem)
from make_golden_romfit import T, LR

N_OBS = 128


def sensor_grid(n):
    """Every second fine free node in both directions of the n x n fine mesh: free nodes are the columns
    i = 1 .. n - 1 of the rows j = 0 .. n, entry j (n - 1) + (i - 1); the sensors sit at odd i, even j."""
    return np.array([j * (n - 1) + (i - 1) for j in range(0, n + 1, 2) for i in range(1, n, 2)], dtype=np.int64)


def make_elbo_partial():
    nc, r, mc, mf, M, W, cdofs, fdofs = c32_physics()
    n = nc * r
    rng = np.random.default_rng(204)
    Nu, bs, Ns = 16, 8, 4
    dz = 16
    torch.manual_seed(0)
    gen = torch.Generator().manual_seed(205)
    enc = CNNEncoder(n, dz, [1, 1], 4, 4, drop_rate=0)
    dec = CNNDecoder(n, dz, (8, 8), 1, 4, [1, 1], False, 4, drop_rate=0., upsample='nearest',
                     force_single_output=False, homoscedastic=False)
    randomize_bn(enc, gen)
    randomize_bn(dec, gen)
    rom = R_ROM.ROM(_Phys(cdofs, fdofs), torch.tensor(M, dtype=torch.float32), torch.float32, 'cpu')
    g = R_comp.ReducedOrderModelOperator(rom, torch.tensor(W, dtype=torch.float32), dtype=torch.float32, device='cpu')
    gp = R_comp.EffectivePropertyMap(dz, M.shape[2], num_hidden_layers=0, independent_X=True, dtype=torch.float32,
                                     device='cpu')
    model = R_gen.GenerativeModel(f=dec, g=g, gp=gp, dtype=torch.float32, device='cpu')
    model.encoder = enc

    Xu = torch.tensor(random_fields(rng, Nu, n), dtype=torch.float32)
    Xs_img = random_fields(rng, Ns, n)
    Xs = torch.tensor(Xs_img, dtype=torch.float32)
    U = rng.uniform(-0.5, 0.5, (Ns, 4))
    Y = np.stack([fem.solve_fom(mf, np.exp(fem.image_to_cells(x)), u) for x, u in zip(Xs_img, U)])
    F = np.stack([fem.f_rom_bc(mc, u) for u in U])
    ds_sup = _DS(X=Xs, Y=torch.tensor(Y, dtype=torch.float32), F_ROM_BC=torch.tensor(F, dtype=torch.float32))
    ds_uns = _DS(X=Xu)
    model.register_datasets({'supervised': ds_sup, 'unsupervised': ds_uns}, None,
                            create_unsupervised_variational_approximation=False)
    with torch.no_grad():
        for q in (model.q_z['supervised'], model.q_X['supervised']):
            q._mean.copy_(torch.tensor(rng.normal(0, 0.5, q._mean.shape)))
            q._logsigma.copy_(torch.tensor(rng.normal(-1.0, 0.3, q._logsigma.shape)))
        g.logsigmas_y.copy_(torch.tensor(rng.normal(-2.0, 0.2, g.logsigmas_y.shape)))
    d_y = Y.shape[1]
    idx = np.sort(rng.choice(d_y, N_OBS, replace=False)).astype(np.int64)
    idx_t = torch.tensor(idx)
    model.preprocess_y_fct = lambda y: y[..., idx_t]

    perm = torch.tensor(rng.permutation(Nu), dtype=torch.long)
    eps = [torch.tensor(rng.normal(size=s), dtype=torch.float32) for s in [(bs, dz), (Ns, dz), (Ns, M.shape[2])]]
    queue = list(eps)

    def fake_randn_like(t, *a, **k):
        e = queue.pop(0)
        assert e.shape == t.shape, (e.shape, t.shape)
        return e.to(dtype=t.dtype)

    class _Writer(object):           # the reference logs every term of the objective to its writer
        def __init__(self):
            self.d = {}

        def add_scalar(self, k, v, global_step=None):
            self.d[k] = float(v.detach()) if hasattr(v, 'detach') else float(v)

    model.writer = _Writer()
    state0 = {k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items()}
    with mock.patch('torch.randperm', lambda N, **k: perm.clone()), mock.patch('torch.randn_like', fake_randn_like):
        elbo = model.elbo(step=0, armortized_bs=bs)
    terms = dict(model.writer.d)
    model.writer = None
    assert not queue
    assert 'objective/supervised_logL_y' in terms, sorted(terms)
    (-elbo).backward()
    gls = g.logsigmas_y.grad.detach().numpy()
    unobserved = np.setdiff1d(np.arange(d_y), idx)
    assert np.all(gls[unobserved] == 0) and np.all(gls[idx] != 0)
    out = {'state.' + k: v for k, v in state0.items()}
    out.update({'grad.' + k: p.grad.detach().numpy() for k, p in model.named_parameters() if p.grad is not None})
    out.update(Xu=Xu.numpy(), Xs=Xs.numpy(), Y=Y.astype(np.float32), F=F.astype(np.float32),
               perm=perm.numpy(), eps_enc=eps[0].numpy(), eps_qz=eps[1].numpy(), eps_qX=eps[2].numpy(),
               elbo=np.float64(elbo.item()), W=W.astype(np.float32), bc_dofs=cdofs, idx=idx,
               cfg=np.array([n, nc, dz, Nu, bs, Ns]))
    for k, v in terms.items():
        out['term.' + k] = np.float64(v)
    path = os.path.join(HERE, 'elbo_partial_c32.npz')
    np.savez_compressed(path, **out)
    size, cap = os.path.getsize(path), os.path.getsize(os.path.join(HERE, 'elbo_c32.npz'))
    assert size <= cap, (size, cap)
    print('partial elbo ok', elbo.item(), 'logL_y', terms['objective/supervised_logL_y'], size, 'bytes')


def make_romfit_partial():
    nc, r, mc, mf, M, W, cdofs, fdofs = c32_physics()
    d = np.load(os.path.join(HERE, 'rom_c32.npz'))
    rom = R_ROM.ROM(_Phys(cdofs, fdofs), torch.tensor(M, dtype=torch.float32), torch.float32, 'cpu')
    g = R_comp.ReducedOrderModelOperator(rom, torch.tensor(W, dtype=torch.float32), dtype=torch.float32, device='cpu')
    ds = _DS(Y=torch.tensor(d['Y']), F_ROM_BC=torch.tensor(d['F']))
    idx = sensor_grid(nc * r)
    idx_t = torch.tensor(idx)
    logX, Y_predict, objective, relerr_list = R_utils.OptimizeEffectiveProperties(
        ds, g, num_iterations=T, lr=LR, verbose=False, y_preprocessor=lambda y: y[..., idx_t])
    assert tuple(Y_predict.shape) == (d['Y'].shape[0], len(idx))
    path = os.path.join(HERE, 'romfit_partial_c32.npz')
    np.savez_compressed(path, T=np.int64(T), lr=np.float64(LR), idx=idx, logX=logX.detach().numpy(),
                        Y_predict=Y_predict.detach().numpy(), objective=np.asarray(objective, dtype=np.float64),
                        relerr_list=np.asarray(relerr_list, dtype=np.float64))
    assert os.path.getsize(path) <= os.path.getsize(os.path.join(HERE, 'elbo_c32.npz'))
    print('partial romfit ok', len(idx), 'sensors', objective[0], objective[-1], relerr_list)


if __name__ == '__main__':
    make_elbo_partial()
    make_romfit_partial()
