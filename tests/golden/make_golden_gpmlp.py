"""ELBO fixture with hidden layers in the effective-property map, from the REFERENCE's own torch modules (run
where the reference exists, never on the GPU box):

    python tests/golden/make_golden_gpmlp.py

elbo_gpmlp_c32.npz: the reference's GenerativeModel.elbo + backward with EffectivePropertyMap(num_hidden_layers = L)
-- gp = the ReLU MLP of lamp/neuralnets.py, widths 16 -> 24 -> 32 (L = 1) and 16 -> 21 -> 26 -> 32 (L = 2) -- at
the highres32 codec (32 x 32, ROM 4 x 4, armortised encoder), B_u = 8 of a pool of 16, N_s = 4, injected noise
and permutation as make_golden_binary.py (same seeds, Gaussian decoder).  Three cases, keys prefixed
'<case>.': 'fx1' free-X L = 1, 'fx2' free-X L = 2, 'lx1' lock-X (independent_X = False) L = 1.  Per case: state
dict, noise, elbo, the per-term scalars the reference logs ('term.objective/...'), all gradients and
'preact_min', the smallest |hidden pre-activation| of the run (asserted >= 1e-4: every hidden ReLU decision of
an fp32 / fp64 re-evaluation is the reference's).  The inputs (fields, Y, F, permutation, physics) are shared by
the cases and stored once.
The reference is imported the way make_golden.py imports it (FEniCS & co. mocked).
"""
import os
from unittest import mock

import numpy as np
import torch

from make_golden import (CNNEncoder, CNNDecoder, R_ROM, R_comp, R_gen, randomize_bn, random_fields, HERE, _Phys, _DS,
                         c32_physics, fem)

PREACT_MIN = 1e-4
CASES = (('fx1', 1, True), ('fx2', 2, True), ('lx1', 1, False))


class _Writer(object):           # the reference logs every term of the objective to its writer
    def __init__(self):
        self.d = {}

    def add_scalar(self, k, v, global_step=None):
        self.d[k] = float(v.detach()) if hasattr(v, 'detach') else float(v)


def run_case(L, independent_X, shared):
    nc, r, mc, mf, M, W, cdofs, fdofs = c32_physics()
    n = nc * r
    rng = np.random.default_rng(104)
    Nu, bs, Ns = 16, 8, 4
    dz = 16
    torch.manual_seed(0)
    gen = torch.Generator().manual_seed(105)
    enc = CNNEncoder(n, dz, [1, 1], 4, 4, drop_rate=0)
    dec = CNNDecoder(n, dz, (8, 8), 1, 4, [1, 1], False, 4, drop_rate=0., upsample='nearest',
                     force_single_output=False, homoscedastic=False)
    randomize_bn(enc, gen)
    randomize_bn(dec, gen)
    rom = R_ROM.ROM(_Phys(cdofs, fdofs), torch.tensor(M, dtype=torch.float32), torch.float32, 'cpu')
    g = R_comp.ReducedOrderModelOperator(rom, torch.tensor(W, dtype=torch.float32), dtype=torch.float32, device='cpu')
    gp = R_comp.EffectivePropertyMap(dz, M.shape[2], num_hidden_layers=L, independent_X=independent_X,
                                     dtype=torch.float32, device='cpu')
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
        # (the q_X rows are drawn in lock-X too, where no q_X exists: the cases share every later draw)
        for q, shape in ((model.q_z['supervised'], (Ns, dz)),
                         (model.q_X['supervised'] if independent_X else None, (Ns, M.shape[2]))):
            mean, logsigma = rng.normal(0, 0.5, shape), rng.normal(-1.0, 0.3, shape)
            if q is not None:
                q._mean.copy_(torch.tensor(mean))
                q._logsigma.copy_(torch.tensor(logsigma))
        g.logsigmas_y.copy_(torch.tensor(rng.normal(-2.0, 0.2, g.logsigmas_y.shape)))

    perm = torch.tensor(rng.permutation(Nu), dtype=torch.long)
    shapes = [(bs, dz), (Ns, dz), (Ns, M.shape[2])]
    eps = [torch.tensor(rng.normal(size=s), dtype=torch.float32) for s in shapes]
    queue = list(eps if independent_X else eps[:2])

    def fake_randn_like(t, *a, **k):
        e = queue.pop(0)
        assert e.shape == t.shape, (e.shape, t.shape)
        return e.to(dtype=t.dtype)

    # the hidden pre-activations of the run: the outputs of fc1 .. fcL
    pre = []
    hooks = [getattr(gp.fc.layers, 'fc%d' % k).register_forward_hook(lambda m, i, o: pre.append(o.detach().clone()))
             for k in range(1, L + 1)]
    model.writer = _Writer()
    state0 = {k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items()}
    with mock.patch('torch.randperm', lambda N, **k: perm.clone()), mock.patch('torch.randn_like', fake_randn_like):
        elbo = model.elbo(step=0, armortized_bs=bs)
    for h in hooks:
        h.remove()
    terms = dict(model.writer.d)
    model.writer = None
    assert not queue and len(pre) == L, (len(queue), len(pre))
    want = {'objective/ARM_unsupervised_DKL_z', 'objective/supervised_DKL_z', 'objective/supervised_logL_y'}
    if independent_X:
        want |= {'objective/supervised_logL_X', 'objective/supervised_entropy_X'}
    assert want <= set(terms), sorted(terms)
    (-elbo).backward()
    preact_min = min(float(a.abs().min()) for a in pre)
    assert preact_min >= PREACT_MIN, preact_min
    out = {'state.' + k: v for k, v in state0.items()}
    out.update({'grad.' + k: p.grad.detach().numpy() for k, p in model.named_parameters() if p.grad is not None})
    out.update(eps_enc=eps[0].numpy(), eps_qz=eps[1].numpy(), elbo=np.float64(elbo.item()),
               preact_min=np.float64(preact_min), L=np.int64(L), independent_X=np.int64(independent_X))
    if independent_X:
        out['eps_qX'] = eps[2].numpy()
    for k, v in terms.items():
        out['term.' + k] = np.float64(v)
    inputs = dict(Xu=Xu.numpy(), Xs=Xs.numpy(), Y=Y.astype(np.float32), F=F.astype(np.float32), U=U, perm=perm.numpy(),
                  M=M.astype(np.float32), W=W.astype(np.float32), bc_dofs=cdofs, cfg=np.array([n, nc, dz, Nu, bs, Ns]))
    if shared:
        for k, v in inputs.items():
            assert np.array_equal(shared[k], v), k
    else:
        shared.update(inputs)
    print('gp mlp L = %d %s: elbo %.6f, min |hidden pre-activation| %.3e'
          % (L, 'freeX' if independent_X else 'lockX', elbo.item(), preact_min))
    return out


def make_elbo_gpmlp():
    out = {}
    for tag, L, indep in CASES:
        case = run_case(L, indep, out)
        out.update({'%s.%s' % (tag, k): v for k, v in case.items()})
    path = os.path.join(HERE, 'elbo_gpmlp_c32.npz')
    np.savez_compressed(path, **out)
    print('elbo_gpmlp_c32.npz', os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) < 1 << 20


if __name__ == '__main__':
    make_elbo_gpmlp()
