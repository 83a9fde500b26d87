"""Test helper: the fp64 CPU oracle of GenerativeModel.elbo with the BINARY decoder (two-phase media;
armortized unsupervised + supervised freeX [+ virtual observables freeX, active or held off], reference
generative.py:232-244,341-392,461-500,546-585), composed from the unchanged oracle/ functions plus the Bernoulli
field term in the logit form.  Test infrastructure only."""
import numpy as np
import torch

from oracle import codec as ocodec
from oracle import elbo as oelbo
from elbo_ref import CODEC, physics, state_of

LOGIT_MAX = 15.0     # parity with the reference's fp32 sigmoid + clamped BCE is claimed below this only
LOG1, LOG10 = float(np.log(1.0)), float(np.log(10.0))


def two_phase(fields):
    """Smooth fields [N, n, n] thresholded at each image's median into log 1 / log 10 (both phases in every image)."""
    fields = np.asarray(fields, dtype=np.float64)
    med = np.median(fields.reshape(len(fields), -1), axis=1)[:, None, None]
    return np.where(fields > med, LOG10, LOG1).astype(np.float32)


def softplus(v):
    """max(v, 0) + log1p(exp(-|v|))."""
    return torch.clamp(v, min=0) + torch.log1p(torch.exp(-v.abs()))


def bernoulli_loglik(X, a, lo=None):
    """Summed Bernoulli log-likelihood of the logit image a for the target bits t = (X != lo), lo = X.min()
    by default (the reference's target == target.min() rule): -softplus(-a) where t, -softplus(a) elsewhere."""
    lo = X.min() if lo is None else lo
    t = X != lo
    return -(torch.where(t, softplus(-a), softplus(a))).sum()


def binary_decoder(dec_p, cfg, masks=None, drops=None):
    """z -> logit image [B, H, W].  oracle.codec.decoder_forward returns channels 0 and 1 of the output conv:
    the one-filter conv3 weight is padded with a zero second filter for the call (its gradient reaches the real
    filter through the concatenation) and channel 0 is the logit."""
    p = dict(dec_p)
    w = p['features.LastTransUp.conv3.weight']
    p['features.LastTransUp.conv3.weight'] = torch.cat([w, torch.zeros_like(w)], 0)
    return lambda z: ocodec.decoder_forward(p, z, 8, cfg['blocks'], cfg['growth'], cfg['f0'], masks, drops)[0]


def _t(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.float64)


def _unsup(st, cfg, n, Xu, eps, mk, dr_enc, dr_u, lo_u, track):
    """generative.py:546-585 with the Bernoulli field term."""
    enc_p = {k[8:]: v for k, v in st.items() if k.startswith('encoder.')}
    dec_p = {k[2:]: v for k, v in st.items() if k.startswith('f.')}
    mean, logsigma = ocodec.encoder_forward(enc_p, Xu, n, cfg['blocks'], cfg['growth'], cfg['f0'], mk.get('enc'), dr_enc)
    a = binary_decoder(dec_p, cfg, mk.get('dec_u'), dr_u)(oelbo.reparam(mean, logsigma, eps))
    track.append(a.detach())
    l = bernoulli_loglik(Xu, a, lo_u)
    kl = oelbo.kl_unit(mean, 2 * logsigma)
    return l - kl, dict(logL_x=l, DKL_z=kl)


def _freeX(st, cfg, key, mask, drops, X, Y, F, eps_z, eps_X, rom, track):
    """generative.py:461-500 (supervised; the active VO term :341-392 is the same algebra on q['vo'] with Y drawn
    from the VO posterior), independent_X = True, with the Bernoulli field term."""
    dec_p = {k[2:]: v for k, v in st.items() if k.startswith('f.')}
    qz = (st['q_z.%s._mean' % key], st['q_z.%s._logsigma' % key])
    qX = (st['q_X.%s._mean' % key], st['q_X.%s._logsigma' % key])
    Z = oelbo.reparam(qz[0], qz[1], eps_z)
    Xt = oelbo.reparam(qX[0], qX[1], eps_X)
    a = binary_decoder(dec_p, cfg, mask, drops)(Z)
    track.append(a.detach())
    l = bernoulli_loglik(X, a)
    mu_X = torch.nn.functional.linear(Z, st['gp.fc.weight'], st['gp.fc.bias'])
    logL_X = oelbo.dgll(Xt, mu_X, 2 * st['gp.logsigmas_X'].expand(Z.shape[0], -1))
    mu_y, ls_y = rom(Xt, F)
    logL_y = oelbo.dgll(Y, mu_y, 2 * ls_y)
    ent, kl = oelbo.entropy(qX[1]), oelbo.kl_unit(qz[0], 2 * qz[1])
    return l + logL_y + logL_X + ent - kl, dict(logL_x=l, logL_X=logL_X, logL_y=logL_y, entropy_X=ent, DKL_z=kl)


def oracle_binary_elbo(st, Xu, Xs, Y, F, eps_enc, eps_qz, eps_qX, nc, r, normalize=False, masks=None, drops=None,
                       lo_u=None, terms=None):
    """ELBO of the armortized + supervised-freeX model with the binary decoder in fp64 from the parameter dict
    ``st`` (reference state_dict names; the Sigmoid module has no state) and fully injected inputs / noise.
    masks: optional {'enc', 'dec_u', 'dec_s'} ReLU decisions of the kernels under test; drops: optional Dropout2d
    channel scales {'enc': {conv: [B_u, C]}, 'dec': {conv: [B_u + N_s, C]}} -- both exactly as
    elbo_ref.oracle_elbo takes them.  lo_u: the unlabelled term's low-phase value (default: the batch's minimum;
    a fused step's is its pool's).  terms: optional dict that receives the two field log-likelihoods, every term
    of the objective as the reference names it ('ARM_unsupervised_<term>', 'supervised_<term>') and the largest
    |logit|."""
    mk, dr = masks or {}, drops or {}
    nu = len(Xu)
    sl = lambda d, a, b: {k: torch.as_tensor(np.asarray(v))[a:b] for k, v in d.items()} if d else None
    n = nc * r
    cfg = CODEC[n] if n in CODEC else CODEC[64]
    M, W, bc = physics(nc, r)
    M, W, bc = _t(M), _t(W), torch.as_tensor(bc)
    rom = lambda x, Fm: oelbo.rom_operator(W, M, bc, x, Fm, st['g.logsigmas_y'])
    track = []
    e1, t_u = _unsup(st, cfg, n, _t(Xu), _t(eps_enc), mk, sl(dr.get('enc'), 0, nu), sl(dr.get('dec'), 0, nu), lo_u, track)
    e2, t_s = _freeX(st, cfg, 'supervised', mk.get('dec_s'), sl(dr.get('dec'), nu, None), _t(Xs), _t(Y), _t(F),
                     _t(eps_qz), _t(eps_qX), rom, track)
    if terms is not None:
        terms.update(logl_u=float(t_u['logL_x'].detach()), logl_s=float(t_s['logL_x'].detach()),
                     logit_max=float(max(a.abs().max() for a in track)))
        terms.update({'ARM_unsupervised_' + k: float(v.detach()) for k, v in t_u.items()})
        terms.update({'supervised_' + k: float(v.detach()) for k, v in t_s.items()})
    if normalize:        # every term divided by its own batch size (generative.py:493-499,571-574)
        e1, e2 = e1 / len(Xu), e2 / len(Xs)
    return e1 + e2


def oracle_binary_fixture_elbo(d, **kw):
    """oracle_binary_elbo on elbo_binary_c32.npz's own inputs / state / noise -> (elbo, {name: grad of -elbo})."""
    n, nc, dz, Nu, bs, Ns = [int(v) for v in d['cfg']]
    st = state_of(d)
    Xu = np.asarray(d['Xu'])[np.asarray(d['perm'][:bs])]
    val = oracle_binary_elbo(st, Xu, d['Xs'], d['Y'], d['F'], d['eps_enc'], d['eps_qz'], d['eps_qX'], nc, n // nc, **kw)
    (-val).backward()
    return float(val.item()), {k: v.grad.numpy() for k, v in st.items() if v.grad is not None}


def binary_vo_fixture(d, n_vo=4):
    """vo_elbo_c32.npz turned into a binary-decoder case with n_vo VO samples: the decoder targets Xu / Xs / Xv
    thresholded into two phases, the output conv's weight cut to its first filter, and the fixture's three VO
    samples extended to n_vo by seeded ones (field and query field from sample 0 -- transposed / reversed --,
    drawn boundary coefficients with their ROM load vector, drawn q_z['vo'] / q_X['vo'] rows and noise rows);
    everything else -- state, noise -- as recorded.  The reference run's values in the fixture do not apply to
    it; the fp64 oracle below does."""
    from oracle import fem
    d = dict(d)
    n, nc, dz, Nu, bs, Ns, Nvo, Nmc = [int(v) for v in d['cfg']]
    rng = np.random.default_rng(404)
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
            w = d['state.%s.vo._mean' % q].shape[1]
            app('state.%s.vo._mean' % q, rng.normal(0, 0.5, (1, w)))
            app('state.%s.vo._logsigma' % q, rng.normal(-1.0, 0.3, (1, w)))
        for k in ('eps3', 'eps4', 'eps5', 'epsh3'):
            app(k, rng.normal(size=(1, d[k].shape[1])))
        for it in range(2):
            for k in ('upd%d.eps_X' % it, 'upd%d.eps_y' % it):
                app(k, rng.normal(size=(Nmc, d[k].shape[1])))
    cfg = d['cfg'].copy()
    cfg[6] = max(n_vo, Nvo)
    d['cfg'] = cfg
    for k in ('Xu', 'Xs', 'Xv'):
        d[k] = two_phase(d[k])
    k = 'state.f.features.LastTransUp.conv3.weight'
    d[k] = np.ascontiguousarray(d[k][:1])
    return d


def oracle_binary_vo_fixture_elbo(d, vo_mean, vo_vars, masks=None, holdoff=False, terms=None):
    """elbo_ref.oracle_vo_fixture_elbo (armortized unsupervised + supervised freeX + virtual observables freeX,
    active or held off) with the binary decoder, on a binary_vo_fixture() dict.  vo_mean / vo_vars: the VO
    posterior the kernels conditioned; masks {'enc', 'dec_u', 'dec_s', 'dec_v'}.  Returns (elbo, {name: grad})."""
    n, nc, dz, Nu, bs, Ns, Nvo, Nmc = [int(v) for v in d['cfg']]
    mk = masks or {}
    cfg = CODEC[n]
    st = state_of(d)
    t = lambda k: _t(d[k])
    M, W, bc = t('M'), t('W'), torch.as_tensor(d['bc_dofs'])
    rom = lambda x, F: oelbo.rom_operator(W, M, bc, x, F, st['g.logsigmas_y'])
    e = lambda i: t('%s%d' % ('epsh' if holdoff else 'eps', i))
    Xu = t('Xu')[torch.as_tensor(d['perm'][:bs])]
    track = []
    e1, t_u = _unsup(st, cfg, n, Xu, e(0), mk, None, None, None, track)
    e2, t_s = _freeX(st, cfg, 'supervised', mk.get('dec_s'), None, t('Xs'), t('Ys'), t('Fs'), e(1), e(2), rom, track)
    l_u, l_s = t_u['logL_x'], t_s['logL_x']
    if holdoff:          # logL_x - KL only (generative.py:349-364)
        qz = (st['q_z.vo._mean'], st['q_z.vo._logsigma'])
        dec_p = {k[2:]: v for k, v in st.items() if k.startswith('f.')}
        a = binary_decoder(dec_p, cfg, mk.get('dec_v'))(oelbo.reparam(qz[0], qz[1], e(3)))
        track.append(a.detach())
        l_v = bernoulli_loglik(t('Xv'), a)
        e3 = l_v - oelbo.kl_unit(qz[0], 2 * qz[1])
    else:
        y = _t(vo_mean) + torch.sqrt(_t(vo_vars)) * e(5)
        e3, t_v = _freeX(st, cfg, 'vo', mk.get('dec_v'), None, t('Xv'), y, t('Fv'), e(3), e(4), rom, track)
        l_v = t_v['logL_x']
    if terms is not None:
        terms.update(logl_u=float(l_u.detach()), logl_s=float(l_s.detach()), logl_v=float(l_v.detach()),
                     logit_max=float(max(a.abs().max() for a in track)))
    val = e1 + e2 + e3
    (-val).backward()
    return float(val.item()), {k: v.grad.numpy() for k, v in st.items() if v.grad is not None}
