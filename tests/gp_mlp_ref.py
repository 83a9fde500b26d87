"""Test helper: the fp64 CPU oracle of GenerativeModel.elbo with hidden layers in the effective-property map
(gp = the ReLU MLP of lamp/neuralnets.py; armortized unsupervised + supervised free-X or lock-X, reference
generative.py:429-500,546-585), composed from the unchanged oracle/ functions -- they take the map as a callable
-- plus the MLP itself.  Test infrastructure only."""
import numpy as np
import torch

from oracle import codec as ocodec
from oracle import elbo as oelbo
from elbo_ref import CODEC, load, physics, state_of

FIXTURE = 'elbo_gpmlp_c32.npz'
CASES = ('fx1', 'fx2', 'lx1')
INPUT_KEYS = ('Xu', 'Xs', 'Y', 'F', 'U', 'perm', 'M', 'W', 'bc_dofs', 'cfg')


def case_of(d, tag):
    """One case of elbo_gpmlp_c32.npz as a fixture dict with elbo_c32.npz's key layout (the shared inputs plus the
    case's 'state.*', 'grad.*', 'term.*', noise and scalars)."""
    out = {k: d[k] for k in INPUT_KEYS}
    out.update({k[len(tag) + 1:]: v for k, v in d.items() if k.startswith(tag + '.')})
    return out


def load_case(tag):
    return case_of(load(FIXTURE), tag)


def mlp_layers(st, prefix='gp.fc.layers.'):
    """[(weight, bias)] of fc1 .. fc{L+1} from a state dict with the reference's names."""
    out, k = [], 1
    while prefix + 'fc%d.weight' % k in st:
        out.append((st[prefix + 'fc%d.weight' % k], st[prefix + 'fc%d.bias' % k]))
        k += 1
    assert out, 'no MLP layers under %s' % prefix
    return out


def mlp(layers, z, pre=None):
    """h_0 = z, h_k = relu(W_k h_{k-1} + b_k), mu_X = W_{L+1} h_L + b_{L+1}.  pre: optional list that receives
    the hidden pre-activations."""
    h = z
    for k, (w, b) in enumerate(layers):
        a = torch.nn.functional.linear(h, w, b)
        if k == len(layers) - 1:
            return a
        if pre is not None:
            pre.append(a.detach())
        h = torch.relu(a)


def _t(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.float64)


def oracle_gpmlp_elbo(st, Xu, Xs, Y, F, eps_enc, eps_qz, eps_qX, nc, r, lockx=False, normalize=False, masks=None,
                      terms=None):
    """ELBO of the armortized + supervised (free-X, or lock-X with eps_qX None) model with the MLP map in fp64 from
    the parameter dict ``st`` and fully injected inputs / noise.  masks: optional {'enc', 'dec_u', 'dec_s'} codec
    ReLU decisions of the kernels under test (as elbo_ref.oracle_elbo).  terms: optional dict that receives every
    term as the reference names it and 'preact_min', the smallest |hidden pre-activation|."""
    mk = masks or {}
    n = nc * r
    cfg = CODEC[n] if n in CODEC else CODEC[64]
    M, W, bc = physics(nc, r)
    M, W, bc = _t(M), _t(W), torch.as_tensor(bc)
    enc_p = {k[8:]: v for k, v in st.items() if k.startswith('encoder.')}
    dec_p = {k[2:]: v for k, v in st.items() if k.startswith('f.')}
    enc = lambda x: ocodec.encoder_forward(enc_p, x, n, cfg['blocks'], cfg['growth'], cfg['f0'], mk.get('enc'))
    dec_u = lambda z: ocodec.decoder_forward(dec_p, z, 8, cfg['blocks'], cfg['growth'], cfg['f0'], mk.get('dec_u'))
    dec_s = lambda z: ocodec.decoder_forward(dec_p, z, 8, cfg['blocks'], cfg['growth'], cfg['f0'], mk.get('dec_s'))
    layers, pre = mlp_layers(st), []
    gp = lambda z: mlp(layers, z, pre)
    rom = lambda x, Fm: oelbo.rom_operator(W, M, bc, x, Fm, st['g.logsigmas_y'])
    qz = (st['q_z.supervised._mean'], st['q_z.supervised._logsigma'])
    e1, t_u = oelbo.elbo_unsupervised_armortized(enc, dec_u, _t(Xu), _t(eps_enc))
    if lockx:
        e2, t_s = oelbo.elbo_supervised_lockX(dec_s, gp, rom, qz, _t(Xs), _t(Y), _t(F), _t(eps_qz))
    else:
        qX = (st['q_X.supervised._mean'], st['q_X.supervised._logsigma'])
        e2, t_s = oelbo.elbo_supervised_freeX(dec_s, gp, st['gp.logsigmas_X'], rom, qz, qX, _t(Xs), _t(Y), _t(F),
                                              _t(eps_qz), _t(eps_qX))
    if terms is not None:
        names = dict(logL_x='logL_x', DKL='DKL_z', logL_y='logL_y', logL_X='logL_X', entropy='entropy_X')
        terms.update({'ARM_unsupervised_' + names[k]: float(v.detach()) for k, v in t_u.items()})
        terms.update({'supervised_' + names[k]: float(v.detach()) for k, v in t_s.items()})
        terms['preact_min'] = min(float(a.abs().min()) for a in pre)
    if normalize:        # every term divided by its own batch size (generative.py:493-499,571-574)
        e1, e2 = e1 / len(Xu), e2 / len(Xs)
    return e1 + e2


def oracle_gpmlp_fixture_elbo(d, **kw):
    """oracle_gpmlp_elbo on one case's own inputs / state / noise -> (elbo, {name: grad of -elbo})."""
    n, nc, dz, Nu, bs, Ns = [int(v) for v in d['cfg']]
    st = state_of(d)
    lockx = not int(d['independent_X'])
    Xu = np.asarray(d['Xu'])[np.asarray(d['perm'][:bs])]
    val = oracle_gpmlp_elbo(st, Xu, d['Xs'], d['Y'], d['F'], d['eps_enc'], d['eps_qz'], None if lockx else d['eps_qX'],
                            nc, n // nc, lockx=lockx, **kw)
    (-val).backward()
    return float(val.item()), {k: v.grad.numpy() for k, v in st.items() if v.grad is not None}


def mlp_vo_fixture(d, n_vo=None, L=1, seed=505):
    """vo_elbo_c32.npz / vo_elbo_lockx_c32.npz turned into a case with L hidden layers in gp: 'state.gp.fc.*' replaced
    by seeded MLP layers under the reference's names (U(-1/sqrt(fan_in), 1/sqrt(fan_in)), torch's Linear init), and,
    with n_vo above the fixture's three VO samples, the VO rows extended as binary_ref.binary_vo_fixture extends
    them (field and query field from sample 0 on -- transposed / reversed --, drawn boundary coefficients with
    their ROM load vector, drawn q rows, drawn update noise).  The reference run's values in the fixture do not
    apply to it."""
    from oracle import fem
    from lamp.neuralnets import linear_decay_widths
    d = dict(d)
    n, nc, dz, Nu, bs, Ns, Nvo, Nmc = [int(v) for v in d['cfg']]
    rng = np.random.default_rng(seed)
    dx = d['state.gp.fc.weight'].shape[0]
    widths = [dz] + linear_decay_widths(dz, dx, L) + [dx]
    for k in ('state.gp.fc.weight', 'state.gp.fc.bias'):
        del d[k]
    for k in range(L + 1):
        a = 1.0 / np.sqrt(widths[k])
        d['state.gp.fc.layers.fc%d.weight' % (k + 1)] = rng.uniform(-a, a, (widths[k + 1], widths[k])).astype(np.float32)
        d['state.gp.fc.layers.fc%d.bias' % (k + 1)] = rng.uniform(-a, a, widths[k + 1]).astype(np.float32)
    n_vo = Nvo if n_vo is None else n_vo
    mc = fem.unit_square_mesh(nc)
    app = lambda k, rows: d.__setitem__(k, np.concatenate([d[k], np.asarray(rows, dtype=d[k].dtype)], 0))
    for i in range(n_vo - Nvo):
        u = rng.uniform(-0.5, 0.5, 4)
        app('Xv', d['Xv'][i:i + 1].transpose(0, 2, 1))
        app('Xv_dg', d['Xv_dg'][i:i + 1, ::-1])
        app('Uv', u[None])
        app('Fv', fem.f_rom_bc(mc, u)[None])
        app('Yv', d['Yv'][i:i + 1])
        for q in ('q_z', 'q_X'):
            if 'state.%s.vo._mean' % q in d:
                w = d['state.%s.vo._mean' % q].shape[1]
                app('state.%s.vo._mean' % q, rng.normal(0, 0.5, (1, w)))
                app('state.%s.vo._logsigma' % q, rng.normal(-1.0, 0.3, (1, w)))
        for it in range(2):
            for k in ('upd%d.eps_X' % it, 'upd%d.eps_y' % it):
                app(k, rng.normal(size=(Nmc, d[k].shape[1])))
    cfg = d['cfg'].copy()
    cfg[6] = n_vo
    d['cfg'] = cfg
    return d
