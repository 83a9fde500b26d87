"""Test helper: the fp64 restatement of partially observed labels -- a 0/1 observation weight per label entry
in the labelled Gaussian likelihood (reference generative.py:49-56,439,473 with
preprocess_y_fct = lambda y: y[..., idx]) and in the optimal-effective-property fit (bottleneck/utils.py:250-282
with a column-selecting y_preprocessor), composed from the unchanged oracle/ functions and tests/romfit_ref.py.
Test infrastructure only."""
import numpy as np
import torch

from oracle import codec as ocodec
from oracle import elbo as oelbo
from elbo_ref import CODEC, physics, state_of
import romfit_ref

LOG2PI = 1.8378770664093453


def _t(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.float64)


def index_weights(idx, d_y, n=None):
    """The 0/1 row [d_y] of an index set (n: repeated to [n, d_y])."""
    w = np.zeros(d_y, dtype=np.float32)
    w[np.asarray(idx)] = 1.0
    return w if n is None else np.repeat(w[None], n, 0)


def dgll_weighted(target, mean, logvars, w):
    """sum_s sum_p w [-1/2 (logvars + (target - mean)^2 exp(-logvars) + log 2 pi)]; an entry with w == 0 is not
    read (target may hold NaN there).  w [d_y] or [N, d_y]; equals oelbo.dgll for w = 1 and oelbo.dgll on the
    selected columns for the 0/1 row of an index set."""
    w = _t(w).expand_as(mean)
    obs = w != 0
    tgt = torch.where(obs, target, mean.detach())
    ll = -0.5 * (logvars + (tgt - mean) ** 2 * torch.exp(-logvars) + LOG2PI)
    return torch.sum(torch.where(obs, w * ll, torch.zeros_like(ll)))


def _codecs(st, n, mk):
    cfg = CODEC[n] if n in CODEC else CODEC[64]
    enc_p = {k[8:]: v for k, v in st.items() if k.startswith('encoder.')}
    dec_p = {k[2:]: v for k, v in st.items() if k.startswith('f.')}
    enc = lambda x: ocodec.encoder_forward(enc_p, x, n, cfg['blocks'], cfg['growth'], cfg['f0'], mk.get('enc'))
    dec = lambda g: (lambda z: ocodec.decoder_forward(dec_p, z, 8, cfg['blocks'], cfg['growth'], cfg['f0'], mk.get(g)))
    return enc, dec


def supervised_freeX(st, dec, rom, key, X, Y, F, eps_z, eps_X, w):
    """oelbo.elbo_supervised_freeX (generative.py:461-500) with the weighted logL_y; w None: every entry."""
    qz = (st['q_z.%s._mean' % key], st['q_z.%s._logsigma' % key])
    qX = (st['q_X.%s._mean' % key], st['q_X.%s._logsigma' % key])
    Z = oelbo.reparam(qz[0], qz[1], eps_z)
    Xt = oelbo.reparam(qX[0], qX[1], eps_X)
    mx, lsx = dec(Z)
    logL_x = oelbo.field_loglik(X, mx, lsx)
    mu_X = torch.nn.functional.linear(Z, st['gp.fc.weight'], st['gp.fc.bias'])
    logL_X = oelbo.dgll(Xt, mu_X, 2 * st['gp.logsigmas_X'].expand(Z.shape[0], -1))
    mu_y, ls_y = rom(Xt, F)
    logL_y = oelbo.dgll(Y, mu_y, 2 * ls_y) if w is None else dgll_weighted(Y, mu_y, 2 * ls_y, w)
    ent, kl = oelbo.entropy(qX[1]), oelbo.kl_unit(qz[0], 2 * qz[1])
    return logL_x + logL_y + logL_X + ent - kl, dict(logL_x=logL_x, logL_X=logL_X, logL_y=logL_y, entropy_X=ent,
                                                     DKL_z=kl)


def supervised_lockX(st, dec, rom, key, X, Y, F, eps_z, w):
    """oelbo.elbo_supervised_lockX (generative.py:429-459) with the weighted logL_y."""
    qz = (st['q_z.%s._mean' % key], st['q_z.%s._logsigma' % key])
    Z = oelbo.reparam(qz[0], qz[1], eps_z)
    mx, lsx = dec(Z)
    logL_x = oelbo.dgll(X, mx, 2 * lsx)
    mu_y, ls_y = rom(torch.nn.functional.linear(Z, st['gp.fc.weight'], st['gp.fc.bias']), F)
    logL_y = oelbo.dgll(Y, mu_y, 2 * ls_y) if w is None else dgll_weighted(Y, mu_y, 2 * ls_y, w)
    kl = oelbo.kl_unit(qz[0], 2 * qz[1])
    return logL_x + logL_y - kl, dict(logL_x=logL_x, logL_y=logL_y, DKL_z=kl)


def oracle_partial_fixture_elbo(d, w, masks=None, lockx=False, terms=None):
    """fp64 ELBO (armortized unsupervised + supervised, freeX or lockX) on an elbo_c32-style fixture's own
    inputs / state / noise with observation weights w ([d_y], [N_s, d_y] or None) on the labelled term ->
    (elbo float, {name: grad of -elbo}).  masks: the kernels' ReLU decisions {'enc', 'dec_u', 'dec_s'}."""
    n, nc, dz, Nu, bs, Ns = [int(v) for v in d['cfg']]
    mk = masks or {}
    st = state_of(d)
    if lockx:
        st = {k: v for k, v in st.items() if not k.startswith('q_X.') and k != 'gp.logsigmas_X'}
    M, W, bc = physics(nc, n // nc)
    M, W, bc = _t(M), _t(W), torch.as_tensor(bc)
    rom = lambda x, Fm: oelbo.rom_operator(W, M, bc, x, Fm, st['g.logsigmas_y'])
    enc, dec = _codecs(st, n, mk)
    Xu = _t(np.asarray(d['Xu'])[np.asarray(d['perm'][:bs])])
    e1, _ = oelbo.elbo_unsupervised_armortized(enc, dec('dec_u'), Xu, _t(d['eps_enc']))
    # (NaN holes of a test's Y are replaced inside dgll_weighted, never read)
    Y = torch.as_tensor(np.asarray(d['Y']), dtype=torch.float64)
    if lockx:
        e2, t_s = supervised_lockX(st, dec('dec_s'), rom, 'supervised', _t(d['Xs']), Y, _t(d['F']), _t(d['eps_qz']), w)
    else:
        e2, t_s = supervised_freeX(st, dec('dec_s'), rom, 'supervised', _t(d['Xs']), Y, _t(d['F']), _t(d['eps_qz']),
                                   _t(d['eps_qX']), w)
    if terms is not None:
        terms.update({'supervised_' + k: float(v.detach()) for k, v in t_s.items()})
    val = e1 + e2
    (-val).backward()
    return float(val.item()), {k: v.grad.numpy() for k, v in st.items() if v.grad is not None}


def rom_loglik(nc, r, x, F, Y, ls, w, loss_scale=1.0):
    """fp64 yardstick of one GPI_ROM_LOGLIK launch with weights: (logL, mu_y [N, d_y], gx [N, n_T] = d(-scale
    logL)/dx, gls [N, d_y] = the per-sample d(-scale logL)/dlogsigma_y rows)."""
    M, W, bc = physics(nc, r)
    M, W, bc = _t(M), _t(W), torch.as_tensor(bc)
    x = _t(x).clone().requires_grad_(True)
    N = x.shape[0]
    lsr = _t(ls)[None].repeat(N, 1).requires_grad_(True)       # a row per sample: per-sample gradients
    u = oelbo.rom_solve(M, torch.exp(x) + 1e-8, _t(F), bc)
    mu = u @ W.t()
    Yt = torch.as_tensor(np.asarray(Y), dtype=torch.float64)
    wt = np.ones((N, mu.shape[1]), dtype=np.float32) if w is None else w
    val = dgll_weighted(Yt, mu, 2 * lsr, wt)
    (-loss_scale * val).backward()
    return float(val.item()), mu.detach().numpy(), x.grad.numpy(), lsr.grad.numpy()


def fit_index(W, M, bc, Y, F, idx, T, lr, dtype=torch.float64, marks=romfit_ref.MARKS):
    """The fit with labels at the nodes idx (shared by the samples): romfit_ref.fit on the selected rows of W
    and columns of Y -- MSELoss after the reference's column-selecting y_preprocessor, i.e.
    J = 1 / (N |idx|) sum |(W u - Y)[idx]|^2."""
    idx = np.asarray(idx)
    return romfit_ref.fit(np.asarray(W)[idx], M, bc, np.asarray(Y)[:, idx], F, T, lr, dtype=dtype, marks=marks)


def fit_weighted(W, M, bc, Y, F, w, T, lr, n_obs=None, dtype=torch.float64, marks=romfit_ref.MARKS):
    """The fit with per-entry weights w [N, d_y] (or [d_y]): T Adam iterations from x = 0 on
    J = 1 / n_obs sum_s sum_p w (W u(x_s) - Y_s)_p^2, n_obs = sum w by default; unobserved entries of Y are
    not read.  Returns romfit_ref.fit's dict (sumsq / ynorm2 over the observed entries)."""
    td = lambda a: torch.as_tensor(np.asarray(a), dtype=dtype)
    W, M, F = td(W), td(M), td(F)
    bc = torch.as_tensor(np.asarray(bc), dtype=torch.long)
    N = len(Y)
    w = td(w).expand(N, W.shape[0])
    obs = w != 0
    Y = torch.where(obs, td(Y), torch.zeros((), dtype=dtype))
    n_obs = float(w.sum()) if n_obs is None else float(n_obs)
    x = torch.zeros(N, M.shape[2], dtype=dtype, requires_grad=True)
    opt = torch.optim.Adam([x], lr=lr)
    ynorm2 = torch.sum(w * Y ** 2, 1)
    objective, sumsq, x_marks = [], [], {}
    x_eval = mu = None
    for n in range(T):
        x_eval = x.detach().clone()
        u = oelbo.rom_solve(M, torch.exp(x) + 1e-8, F, bc)
        mu = u @ W.t()
        ss = torch.sum(w * (mu - Y) ** 2, 1)
        J = torch.sum(ss) / n_obs
        opt.zero_grad()
        J.backward()
        objective.append(J.item())
        sumsq.append(ss.detach())
        opt.step()
        if n + 1 in marks:
            x_marks[n + 1] = x.detach().clone().numpy()
    return dict(x=x.detach().numpy(), x_marks=x_marks, x_eval=None if x_eval is None else x_eval.numpy(),
                Y_predict=None if mu is None else mu.detach().numpy(),
                objective=np.asarray(objective, dtype=np.float64),
                sumsq=torch.stack(sumsq).numpy() if sumsq else np.zeros((0, N)), ynorm2=ynorm2.numpy())


def vo_fixture(d, n_vo=4):
    """vo_elbo_c32.npz with its three VO samples extended to n_vo by seeded ones, as binary_ref.binary_vo_fixture
    extends them (field and query field from sample 0 -- transposed / reversed --, drawn boundary coefficients
    with their ROM load vector, drawn q_z['vo'] / q_X['vo'] rows and noise rows); everything else as recorded.
    The reference run's values in the fixture do not apply to it; the fp64 restatement below does."""
    from oracle import fem
    d = dict(d)
    n, nc, dz, Nu, bs, Ns, Nvo, Nmc = [int(v) for v in d['cfg']]
    rng = np.random.default_rng(405)
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
            wd = d['state.%s.vo._mean' % q].shape[1]
            app('state.%s.vo._mean' % q, rng.normal(0, 0.5, (1, wd)))
            app('state.%s.vo._logsigma' % q, rng.normal(-1.0, 0.3, (1, wd)))
        for k in ('eps3', 'eps4', 'eps5', 'epsh3'):
            app(k, rng.normal(size=(1, d[k].shape[1])))
        for it in range(2):
            for k in ('upd%d.eps_X' % it, 'upd%d.eps_y' % it):
                app(k, rng.normal(size=(Nmc, d[k].shape[1])))
    cfg = d['cfg'].copy()
    cfg[6] = max(n_vo, Nvo)
    d['cfg'] = cfg
    return d


def oracle_partial_vo_fixture_elbo(d, vo_mean, vo_vars, w, masks=None):
    """elbo_ref.oracle_vo_fixture_elbo (armortized unsupervised + supervised freeX + active virtual observables
    freeX) with observation weights w on the SUPERVISED term only -- virtual observables are complete by
    construction -- on a vo_fixture() dict.  vo_mean / vo_vars: the VO posterior the kernels conditioned; masks
    {'enc', 'dec_u', 'dec_s', 'dec_v'}.  Returns (elbo, {name: grad of -elbo})."""
    n, nc, dz, Nu, bs, Ns, Nvo, Nmc = [int(v) for v in d['cfg']]
    mk = masks or {}
    st = state_of(d)
    t = lambda k: _t(d[k])
    M, W, bc = t('M'), t('W'), torch.as_tensor(d['bc_dofs'])
    rom = lambda x, F: oelbo.rom_operator(W, M, bc, x, F, st['g.logsigmas_y'])
    enc, dec = _codecs(st, n, mk)
    Xu = t('Xu')[torch.as_tensor(d['perm'][:bs])]
    e1, _ = oelbo.elbo_unsupervised_armortized(enc, dec('dec_u'), Xu, t('eps0'))
    Ys = torch.as_tensor(np.asarray(d['Ys']), dtype=torch.float64)
    e2, _ = supervised_freeX(st, dec('dec_s'), rom, 'supervised', t('Xs'), Ys, t('Fs'), t('eps1'), t('eps2'), w)
    y = _t(vo_mean) + torch.sqrt(_t(vo_vars)) * t('eps5')
    e3, _ = supervised_freeX(st, dec('dec_v'), rom, 'vo', t('Xv'), y, t('Fv'), t('eps3'), t('eps4'), None)
    val = e1 + e2 + e3
    (-val).backward()
    return float(val.item()), {k: v.grad.numpy() for k, v in st.items() if v.grad is not None}
