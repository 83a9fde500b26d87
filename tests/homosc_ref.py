"""Test helper: the fp64 CPU oracle of GenerativeModel.elbo with the HOMOSCEDASTIC decoder (one mean channel and the
learned log-sigma plane f.logsigma [H, W] shared by every sample, reference Decoder.py:204-212,271-285; armortized
unsupervised + supervised freeX [+ virtual observables freeX, active or held off], generative.py:232-239,341-392,
461-500,546-585), composed from the unchanged oracle/ functions: the decoder callable returns (mean, plane expanded
over the batch) and oracle.elbo scores it with its diagonal Gaussian (dgll) as it scores the two-channel decoder.
Test infrastructure only."""
import numpy as np
import torch

from oracle import codec as ocodec
from oracle import elbo as oelbo
from elbo_ref import CODEC, physics, state_of

TERM_NAMES = dict(logL_x='logL_x', logL_X='logL_X', logL_y='logL_y', DKL='DKL_z', entropy='entropy_X')


def homosc_decoder(dec_p, cfg, masks=None, drops=None):
    """z -> (mean [B, H, W], log sigma [B, H, W]).  oracle.codec.decoder_forward returns channels 0 and 1 of the
    output conv: the one-filter conv3 weight is padded with a zero second filter for the call (its gradient reaches
    the real filter through the concatenation), channel 0 is the mean, and the log sigma is the plane expanded over
    the batch (its gradient sums over the samples)."""
    p = {k: v for k, v in dec_p.items() if k != 'logsigma'}
    w = p['features.LastTransUp.conv3.weight']
    p['features.LastTransUp.conv3.weight'] = torch.cat([w, torch.zeros_like(w)], 0)
    plane = dec_p['logsigma']

    def dec(z):
        mean = ocodec.decoder_forward(p, z, 8, cfg['blocks'], cfg['growth'], cfg['f0'], masks, drops)[0]
        return mean, plane.expand(mean.shape)
    return dec


def _t(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.float64)


def _dec_params(st):
    return {k[2:]: v for k, v in st.items() if k.startswith('f.')}


def oracle_homosc_elbo(st, Xu, Xs, Y, F, eps_enc, eps_qz, eps_qX, nc, r, normalize=False, masks=None, drops=None,
                       log_field=True, terms=None):
    """ELBO of the armortized + supervised-freeX model with the homoscedastic decoder in fp64 from the parameter
    dict ``st`` (reference state_dict names, 'f.logsigma' the plane) and fully injected inputs / noise.
    masks: optional {'enc', 'dec_u', 'dec_s'} ReLU decisions of the kernels under test; drops: optional Dropout2d
    channel scales {'enc': {conv: [B_u, C]}, 'dec': {conv: [B_u + N_s, C]}} -- both exactly as elbo_ref.oracle_elbo
    takes them.  log_field: reconstruct_log_eff_property.  terms: optional dict that receives the two field
    log-likelihoods and every term of the objective as the reference names it ('ARM_unsupervised_<term>',
    'supervised_<term>')."""
    mk, dr = masks or {}, drops or {}
    nu = len(Xu)
    sl = lambda d, a, b: {k: torch.as_tensor(np.asarray(v))[a:b] for k, v in d.items()} if d else None
    n = nc * r
    cfg = CODEC[n] if n in CODEC else CODEC[64]
    M, W, bc = physics(nc, r)
    M, W, bc = _t(M), _t(W), torch.as_tensor(bc)
    enc_p = {k[8:]: v for k, v in st.items() if k.startswith('encoder.')}
    dec_p = _dec_params(st)
    enc = lambda x: ocodec.encoder_forward(enc_p, x, n, cfg['blocks'], cfg['growth'], cfg['f0'], mk.get('enc'),
                                           sl(dr.get('enc'), 0, nu))
    dec_u = homosc_decoder(dec_p, cfg, mk.get('dec_u'), sl(dr.get('dec'), 0, nu))
    dec_s = homosc_decoder(dec_p, cfg, mk.get('dec_s'), sl(dr.get('dec'), nu, None))
    gp = lambda z: torch.nn.functional.linear(z, st['gp.fc.weight'], st['gp.fc.bias'])
    rom = lambda x, Fm: oelbo.rom_operator(W, M, bc, x, Fm, st['g.logsigmas_y'])
    e1, t_u = oelbo.elbo_unsupervised_armortized(enc, dec_u, _t(Xu), _t(eps_enc), log_field)
    e2, t_s = oelbo.elbo_supervised_freeX(
        dec_s, gp, st['gp.logsigmas_X'], rom, (st['q_z.supervised._mean'], st['q_z.supervised._logsigma']),
        (st['q_X.supervised._mean'], st['q_X.supervised._logsigma']), _t(Xs), _t(Y), _t(F), _t(eps_qz), _t(eps_qX),
        log_field)
    if terms is not None:
        terms.update(logl_u=float(t_u['logL_x'].detach()), logl_s=float(t_s['logL_x'].detach()))
        terms.update({'ARM_unsupervised_' + TERM_NAMES[k]: float(v.detach()) for k, v in t_u.items()})
        terms.update({'supervised_' + TERM_NAMES[k]: float(v.detach()) for k, v in t_s.items()})
    if normalize:        # every term divided by its own batch size (generative.py:493-499,571-574)
        e1, e2 = e1 / len(Xu), e2 / len(Xs)
    return e1 + e2


def oracle_homosc_fixture_elbo(d, **kw):
    """oracle_homosc_elbo on elbo_homosc_c32.npz's own inputs / state / noise -> (elbo, {name: grad of -elbo})."""
    n, nc, dz, Nu, bs, Ns = [int(v) for v in d['cfg']]
    st = state_of(d)
    Xu = np.asarray(d['Xu'])[np.asarray(d['perm'][:bs])]
    val = oracle_homosc_elbo(st, Xu, d['Xs'], d['Y'], d['F'], d['eps_enc'], d['eps_qz'], d['eps_qX'], nc, n // nc, **kw)
    (-val).backward()
    return float(val.item()), {k: v.grad.numpy() for k, v in st.items() if v.grad is not None}


def homosc_vo_fixture(d, n_vo=4):
    """vo_elbo_c32.npz turned into a homoscedastic-decoder case with n_vo VO samples: the output conv's weight cut
    to its first filter, a seeded plane f.logsigma ~ N(-1, 0.3) added to the state, and the fixture's three VO
    samples extended to n_vo by seeded ones (field and query field from sample 0 -- transposed / reversed --, drawn
    boundary coefficients with their ROM load vector, drawn q_z['vo'] / q_X['vo'] rows and noise rows, as
    binary_ref.binary_vo_fixture extends them); everything else -- state, fields, noise -- as recorded.  The
    reference run's values in the fixture do not apply to it; the fp64 oracle below does."""
    from oracle import fem
    d = dict(d)
    n, nc, dz, Nu, bs, Ns, Nvo, Nmc = [int(v) for v in d['cfg']]
    rng = np.random.default_rng(504)
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
    k = 'state.f.features.LastTransUp.conv3.weight'
    d[k] = np.ascontiguousarray(d[k][:1])
    d['state.f.logsigma'] = rng.normal(-1.0, 0.3, (n, n)).astype(np.float32)
    return d


def oracle_homosc_vo_fixture_elbo(d, vo_mean, vo_vars, masks=None, holdoff=False, log_field=True, terms=None):
    """elbo_ref.oracle_vo_fixture_elbo (armortized unsupervised + supervised freeX + virtual observables freeX,
    active or held off) with the homoscedastic decoder, on a homosc_vo_fixture() dict.  vo_mean / vo_vars: the VO
    posterior the kernels conditioned; masks {'enc', 'dec_u', 'dec_s', 'dec_v'}.  Returns (elbo, {name: grad})."""
    n, nc, dz, Nu, bs, Ns, Nvo, Nmc = [int(v) for v in d['cfg']]
    mk = masks or {}
    cfg = CODEC[n]
    st = state_of(d)
    t = lambda k: _t(d[k])
    M, W, bc = t('M'), t('W'), torch.as_tensor(d['bc_dofs'])
    enc_p = {k[8:]: v for k, v in st.items() if k.startswith('encoder.')}
    dec_p = _dec_params(st)
    enc = lambda x: ocodec.encoder_forward(enc_p, x, n, cfg['blocks'], cfg['growth'], cfg['f0'], mk.get('enc'))
    dec = {g: homosc_decoder(dec_p, cfg, mk.get(g)) for g in ('dec_u', 'dec_s', 'dec_v')}
    gp = lambda z: torch.nn.functional.linear(z, st['gp.fc.weight'], st['gp.fc.bias'])
    rom = lambda x, F: oelbo.rom_operator(W, M, bc, x, F, st['g.logsigmas_y'])
    qz = lambda key: (st['q_z.%s._mean' % key], st['q_z.%s._logsigma' % key])
    qx = lambda key: (st['q_X.%s._mean' % key], st['q_X.%s._logsigma' % key])
    e = lambda i: t('%s%d' % ('epsh' if holdoff else 'eps', i))
    Xu = t('Xu')[torch.as_tensor(d['perm'][:bs])]
    e1, t_u = oelbo.elbo_unsupervised_armortized(enc, dec['dec_u'], Xu, e(0), log_field)
    e2, t_s = oelbo.elbo_supervised_freeX(dec['dec_s'], gp, st['gp.logsigmas_X'], rom, qz('supervised'),
                                          qx('supervised'), t('Xs'), t('Ys'), t('Fs'), e(1), e(2), log_field)
    if holdoff:          # logL_x - KL only (generative.py:349-364)
        mx, lsx = dec['dec_v'](oelbo.reparam(*qz('vo'), e(3)))
        l_v = oelbo.field_loglik(t('Xv'), mx, lsx, log_field)
        e3 = l_v - oelbo.kl_unit(qz('vo')[0], 2 * qz('vo')[1])
    else:
        y = _t(vo_mean) + torch.sqrt(_t(vo_vars)) * e(5)
        e3, t_v = oelbo.elbo_supervised_freeX(dec['dec_v'], gp, st['gp.logsigmas_X'], rom, qz('vo'), qx('vo'),
                                              t('Xv'), y, t('Fv'), e(3), e(4), log_field)
        l_v = t_v['logL_x']
    if terms is not None:
        terms.update(logl_u=float(t_u['logL_x'].detach()), logl_s=float(t_s['logL_x'].detach()),
                     logl_v=float(l_v.detach()))
    val = e1 + e2 + e3
    (-val).backward()
    return float(val.item()), {k: v.grad.numpy() for k, v in st.items() if v.grad is not None}
