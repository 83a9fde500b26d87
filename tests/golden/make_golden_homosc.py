"""Homoscedastic-decoder ELBO fixture from the REFERENCE's own torch modules (run where the reference exists,
never on the GPU box):

    python tests/golden/make_golden_homosc.py

elbo_homosc_c32.npz: the reference's GenerativeModel.elbo + backward with the HOMOSCEDASTIC CNNDecoder (one mean
channel and the learned log-sigma plane f.logsigma [H, W] expanded over the batch, Decoder.py:204-212,271-285;
scored by the diagonal Gaussian of generative.py:232-239) at the highres32 codec (32 x 32, ROM 4 x 4, armortised
encoder, freeX), B_u = 8 of a pool of 16, N_s = 4, injected noise and permutation as make_golden.py's make_elbo.
Two runs on ONE state and one set of noise: reconstruct_log_eff_property True ('log.*': the Gaussian of the log
field) and False ('exp.*': of the exponentiated field).  f.logsigma is initialised ~ N(-1, 0.3): a zero plane's
gradient would be the trivial one.
Contents: inputs, noise, state dict, and per run the elbo, the per-term scalars the reference logs
('<run>.term.objective/...'), the decoder log-likelihood of the two decoder calls and all gradients.
The reference is imported the way make_golden.py imports it (FEniCS & co. mocked).
"""
import os
from unittest import mock

import numpy as np
import torch

from make_golden import (CNNEncoder, CNNDecoder, R_ROM, R_comp, R_gen, randomize_bn, random_fields, HERE, _Phys, _DS,
                         c32_physics, fem)


def make_elbo_homosc():
    nc, r, mc, mf, M, W, cdofs, fdofs = c32_physics()
    n = nc * r
    rng = np.random.default_rng(204)
    Nu, bs, Ns = 16, 8, 4
    dz = 16
    torch.manual_seed(0)
    gen = torch.Generator().manual_seed(205)
    enc = CNNEncoder(n, dz, [1, 1], 4, 4, drop_rate=0)
    dec = CNNDecoder(n, dz, (8, 8), 1, 4, [1, 1], False, 4, drop_rate=0., upsample='nearest',
                     force_single_output=False, homoscedastic=True)
    assert list(dec.state_dict())[0] == 'logsigma' and tuple(dec.logsigma.shape) == (n, n)
    randomize_bn(enc, gen)
    randomize_bn(dec, gen)
    rom = R_ROM.ROM(_Phys(cdofs, fdofs), torch.tensor(M, dtype=torch.float32), torch.float32, 'cpu')
    g = R_comp.ReducedOrderModelOperator(rom, torch.tensor(W, dtype=torch.float32), dtype=torch.float32, device='cpu')
    gp = R_comp.EffectivePropertyMap(dz, M.shape[2], num_hidden_layers=0, independent_X=True, dtype=torch.float32,
                                     device='cpu')
    model = R_gen.GenerativeModel(f=dec, g=g, gp=gp, dtype=torch.float32, device='cpu')
    model.encoder = enc

    Xu_img = random_fields(rng, Nu, n)
    Xs_img = random_fields(rng, Ns, n)
    Xu = torch.tensor(Xu_img, dtype=torch.float32)
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
        dec.logsigma.copy_(torch.tensor(rng.normal(-1.0, 0.3, dec.logsigma.shape)))

    perm = torch.tensor(rng.permutation(Nu), dtype=torch.long)
    eps = [torch.tensor(rng.normal(size=s), dtype=torch.float32) for s in [(bs, dz), (Ns, dz), (Ns, M.shape[2])]]

    class _Writer(object):           # the reference logs every term of the objective to its writer
        def __init__(self):
            self.d = {}

        def add_scalar(self, k, v, global_step=None):
            self.d[k] = float(v.detach()) if hasattr(v, 'detach') else float(v)

    state0 = {k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items()}
    out = {'state.' + k: v for k, v in state0.items()}
    # the decoder's state-dict keys in the reference's order (an .npz keeps no order of its own): f.logsigma first
    out['state_keys_f'] = np.array([k for k in state0 if k.startswith('f.')])
    assert out['state_keys_f'][0] == 'f.logsigma'
    real_lik = model.random_field_likelihood
    for tag, log_field in (('log', True), ('exp', False)):
        model.set('reconstruct_log_eff_property', log_field)
        queue = list(eps)

        def fake_randn_like(t, *a, **k):
            e = queue.pop(0)
            assert e.shape == t.shape, (e.shape, t.shape)
            return e.to(dtype=t.dtype)

        logl = []

        def spy_lik(predict, target):
            assert isinstance(predict, tuple) and predict[0].shape == predict[1].shape, 'mean and the expanded plane'
            v = real_lik(predict, target)
            logl.append(float(v.detach().sum()))
            return v

        model.random_field_likelihood = spy_lik
        model.writer = _Writer()
        model.zero_grad()
        for p in model.parameters():
            p.grad = None
        with mock.patch('torch.randperm', lambda N, **k: perm.clone()), mock.patch('torch.randn_like', fake_randn_like):
            elbo = model.elbo(step=0, armortized_bs=bs)
        terms = dict(model.writer.d)
        model.writer = None
        model.random_field_likelihood = real_lik
        assert not queue and len(logl) == 2
        (-elbo).backward()
        assert dec.logsigma.grad is not None and float(dec.logsigma.grad.abs().max()) > 0
        out.update({'%s.grad.%s' % (tag, k): p.grad.detach().numpy().copy() for k, p in model.named_parameters()
                    if p.grad is not None})
        out['%s.elbo' % tag] = np.float64(elbo.item())
        out['%s.logl_field' % tag] = np.array(logl)
        for k, v in terms.items():
            out['%s.term.%s' % (tag, k)] = np.float64(v)
        print('homoscedastic elbo', tag, elbo.item(), 'field logL', logl)
    # the state is unchanged by the runs (no optimiser step, train-mode BN touches running buffers only)
    for k, v in model.state_dict().items():
        if not k.endswith(('running_mean', 'running_var', 'num_batches_tracked')):
            assert np.array_equal(v.detach().numpy(), state0[k]), k
    out.update(Xu=Xu.numpy(), Xs=Xs.numpy(), Y=Y.astype(np.float32), F=F.astype(np.float32), U=U,
               perm=perm.numpy(), eps_enc=eps[0].numpy(), eps_qz=eps[1].numpy(), eps_qX=eps[2].numpy(),
               M=M.astype(np.float32), W=W.astype(np.float32), bc_dofs=cdofs, cfg=np.array([n, nc, dz, Nu, bs, Ns]))
    path = os.path.join(HERE, 'elbo_homosc_c32.npz')
    np.savez_compressed(path, **out)
    print('homoscedastic fixture ok', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    make_elbo_homosc()
