"""Binary-field (two-phase media) ELBO fixture from the REFERENCE's own torch modules (run where the
reference exists, never on the GPU box):

    python tests/golden/make_golden_binary.py

elbo_binary_c32.npz: the reference's GenerativeModel.elbo + backward with the BINARY CNNDecoder (one
output channel + Sigmoid, Decoder.py:204-207,240-241; Bernoulli likelihood generative.py:240-244) at the
highres32 codec (32 x 32, ROM 4 x 4, armortised encoder, freeX), B_u = 8 of a pool of 16, N_s = 4, injected
noise and permutation as make_golden.py's make_elbo.  Fields are two-valued (log 1 / log 10: the seeded
smooth fields of elbo_ref.random_fields thresholded at their median), every image holds both phases.
Contents: inputs, noise, state dict, elbo, the per-term scalars the reference logs ('term.objective/...': field
log-likelihoods, KL, logL_y, logL_X, entropy), the decoder log-likelihood of the two terms, all gradients and
the largest |logit| (asserted < 15: above ~16.7 the reference's fp32 sigmoid rounds to 1 and torch clamps
the log at -100, where the native logit form deliberately differs).
The reference is imported the way make_golden.py imports it (FEniCS & co. mocked).
"""
import os
from unittest import mock

import numpy as np
import torch

from make_golden import (CNNEncoder, CNNDecoder, R_ROM, R_comp, R_gen, randomize_bn, random_fields, HERE, _Phys, _DS,
                         c32_physics, fem)

LO, HI = np.log(1.0), np.log(10.0)
LOGIT_MAX = 15.0


def two_phase(fields):
    """Threshold each smooth field at its own median: both phases in every image."""
    med = np.median(fields.reshape(len(fields), -1), axis=1)[:, None, None]
    out = np.where(fields > med, HI, LO)
    for img in out:
        assert (img == LO).any() and (img == HI).any(), 'an image holds one phase only'
    return out


def make_elbo_binary():
    nc, r, mc, mf, M, W, cdofs, fdofs = c32_physics()
    n = nc * r
    rng = np.random.default_rng(104)
    Nu, bs, Ns = 16, 8, 4
    dz = 16
    torch.manual_seed(0)
    gen = torch.Generator().manual_seed(105)
    enc = CNNEncoder(n, dz, [1, 1], 4, 4, drop_rate=0)
    dec = CNNDecoder(n, dz, (8, 8), 1, 4, [1, 1], True, 4, drop_rate=0., upsample='nearest',
                     force_single_output=False, homoscedastic=False)
    randomize_bn(enc, gen)
    randomize_bn(dec, gen)
    rom = R_ROM.ROM(_Phys(cdofs, fdofs), torch.tensor(M, dtype=torch.float32), torch.float32, 'cpu')
    g = R_comp.ReducedOrderModelOperator(rom, torch.tensor(W, dtype=torch.float32), dtype=torch.float32, device='cpu')
    gp = R_comp.EffectivePropertyMap(dz, M.shape[2], num_hidden_layers=0, independent_X=True, dtype=torch.float32,
                                     device='cpu')
    model = R_gen.GenerativeModel(f=dec, g=g, gp=gp, dtype=torch.float32, device='cpu')
    model.encoder = enc

    Xu_img = two_phase(random_fields(rng, Nu, n))
    Xs_img = two_phase(random_fields(rng, Ns, n))
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

    perm = torch.tensor(rng.permutation(Nu), dtype=torch.long)
    eps = [torch.tensor(rng.normal(size=s), dtype=torch.float32) for s in [(bs, dz), (Ns, dz), (Ns, M.shape[2])]]
    queue = list(eps)

    def fake_randn_like(t, *a, **k):
        e = queue.pop(0)
        assert e.shape == t.shape, (e.shape, t.shape)
        return e.to(dtype=t.dtype)

    # the logit images (LastTransUp's output, before the Sigmoid module) and the likelihood of each decoder call
    logits, logl = [], []
    hook = dec.features.LastTransUp.register_forward_hook(lambda m, i, o: logits.append(o.detach().clone()))
    real_lik = model.random_field_likelihood

    def spy_lik(predict, target):
        assert not isinstance(predict, tuple), 'the binary decoder returns the probability image'
        v = real_lik(predict, target)
        logl.append(float(v.detach().sum()))
        return v

    model.random_field_likelihood = spy_lik

    class _Writer(object):           # the reference logs every term of the objective to its writer
        def __init__(self):
            self.d = {}

        def add_scalar(self, k, v, global_step=None):
            self.d[k] = float(v.detach()) if hasattr(v, 'detach') else float(v)

    model.writer = _Writer()
    state0 = {k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items()}
    with mock.patch('torch.randperm', lambda N, **k: perm.clone()), mock.patch('torch.randn_like', fake_randn_like):
        elbo = model.elbo(step=0, armortized_bs=bs)
    hook.remove()
    terms = dict(model.writer.d)
    model.writer = None
    assert {'objective/ARM_unsupervised_DKL_z', 'objective/supervised_DKL_z', 'objective/supervised_logL_y',
            'objective/supervised_logL_X', 'objective/supervised_entropy_X'} <= set(terms), sorted(terms)
    assert not queue and len(logits) == 2 and len(logl) == 2
    (-elbo).backward()
    logit_max = max(float(a.abs().max()) for a in logits)
    assert logit_max < LOGIT_MAX, logit_max
    out = {'state.' + k: v for k, v in state0.items()}
    out.update({'grad.' + k: p.grad.detach().numpy() for k, p in model.named_parameters() if p.grad is not None})
    out.update(Xu=Xu.numpy(), Xs=Xs.numpy(), Y=Y.astype(np.float32), F=F.astype(np.float32), U=U,
               perm=perm.numpy(), eps_enc=eps[0].numpy(), eps_qz=eps[1].numpy(), eps_qX=eps[2].numpy(),
               elbo=np.float64(elbo.item()), logl_field=np.array(logl), logit_max=np.float64(logit_max),
               M=M.astype(np.float32), W=W.astype(np.float32), bc_dofs=cdofs, cfg=np.array([n, nc, dz, Nu, bs, Ns]))
    for k, v in terms.items():       # per-term scalars: 'term.objective/<term>' as vo_elbo_c32.npz keeps them
        out['term.' + k] = np.float64(v)
    path = os.path.join(HERE, 'elbo_binary_c32.npz')
    np.savez_compressed(path, **out)
    print('binary elbo ok', elbo.item(), 'field logL', logl, 'max |logit|', logit_max, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    make_elbo_binary()
