"""Plain torch reference of the dense head (gpi_head_forward / gpi_head_backward / gpi_outer_gemm), fp64 on the CPU.

Written from the header comment of gpi_head_desc (include/gpi.h) and the reference lines it cites:
    encoder FC -> ReLU -> (mu, logsigma) heads            Encoder.py:175-182, codec.py:495-504
    z = mu + exp(logsigma) eps                            bottleneck/utils.py:216-219, components.py:167-172
    KL = -1/2 sum(1 + 2 logsigma - mu^2 - exp(2 logsigma))  bottleneck/utils.py:246-248, components.py:192-193
    lat = latent_map(z)                                   Decoder.py:213
    mu_X = gp(z) = fc(z), logsigma_X a parameter vector   components.py:201-256
    X~ = mean + exp(logsigma) eps of q_X, or gp(z) itself (lockX)   components.py:167-172, generative.py:429-459
    logL_X = sum -1/2 (2 ls_X + ((X~ - mu_X) / exp(ls_X))^2 + log 2 pi)   bottleneck/utils.py:231-243
    H = sum logsigma of q_X (its constant N/2 (log 2 pi + 1) is added by the caller)   components.py:195-197
The backward is autograd of
    J = kl_scale_enc KL_enc + kl_scale_q KL_q1 + kl_scale_q2 KL_q2 - lx_scale (logL_X1 + H1) - lx_scale2 (logL_X2 + H2)
        + <glat, lat> (or <gz, z> without the latent map) + <gxs, X~>,
so the shared-weight gradients gpi_outer_gemm forms are d J / d weight, the per-sample deltas the workspace holds
(gmux, dzmu, dzls, dhpre, gfeat) the gradients of the intermediate nodes.

Without GPI_HEAD_REPARAM the encoder samples' z is the caller's (workspace z); the backward then hands dJ/dz to mu
and takes the caller's stored dzls as dJ/dlogsigma (the stand-alone encoder engine: GPI_HEAD_ENC alone, dJ/dz = gz;
the stand-alone decoder engine: GPI_HEAD_LATENT alone).

A workspace region is returned whole, NaN in the rows the mode does not write.  `wrong` selects a deliberately
wrong variant (tests/test_head_cases_plan.py: what the comparison must notice); `dtype` the evaluation precision.
"""
import numpy as np
import torch

ENC, REPARAM, QZ, LATENT, GP, LOCKX = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20
LOG2PI = 1.8378770664093453

TERMS = ('kl_enc', 'kl_q', 'logl_x', 'ent', 'kl_q2', 'logl_x2', 'ent2')      # terms[0..3], terms2[0..2]
FWD_REGIONS = ('hpre', 'zmu', 'zls', 'z', 'lat', 'mux', 'xs')
BWD_REGIONS = ('gmux', 'dzmu', 'dzls', 'dhpre', 'gfeat')
WRONG = ('seg2_scales', 'seg2_rows', 'drop_last', 'no_relu_mask', 'no_entropy', 'holdoff_gp')


def kl_rows(mu, ls):
    return -0.5 * (1 + 2 * ls - mu ** 2 - torch.exp(2 * ls)).sum(1)


def head_reference(c, dtype=torch.float64, wrong=None):
    """c: a head_cases.Case (widths, counts, flags, scales, params, inputs as fp32 arrays).  Returns a dict of
    float64 arrays: the regions of FWD_REGIONS / BWD_REGIONS, 'terms' [7], and 'grad:<param>' per parameter."""
    assert wrong is None or wrong in WRONG
    T = lambda a: torch.tensor(np.asarray(a, dtype=np.float64), dtype=dtype)
    ne, nq, nq2 = c.n_enc, c.n_q, c.n_q2
    B, nqt = ne + nq + nq2, nq + nq2
    df, dz, dl, dx = c.widths
    f1, f2 = c.flags, c.flags2
    par = {k: T(v).requires_grad_() for k, v in c.params.items()}
    x = {k: T(v) for k, v in c.inputs.items()}
    w = torch.ones(B, dtype=dtype)                     # sample weights: 1 (drop_last: one sample left out)
    if wrong == 'drop_last':
        w[c.drop_sample] = 0
    nan = lambda *s: torch.full(s, float('nan'), dtype=dtype)
    out = {k: nan(*s) for k, s in (('hpre', (ne, df)), ('dhpre', (ne, df)), ('gfeat', (ne, df)), ('zmu', (B, dz)),
                                   ('zls', (B, dz)), ('z', (B, dz)), ('dzmu', (B, dz)), ('dzls', (B, dz)),
                                   ('lat', (B, dl)), ('mux', (nqt, dx)), ('xs', (nqt, dx)), ('gmux', (nqt, dx)))}
    terms = {k: torch.zeros((), dtype=dtype) for k in TERMS}
    J = torch.zeros((), dtype=dtype)
    zs, nodes = [], {}
    # ---- encoder samples
    if ne:
        we = w[:ne]
        if f1 & ENC:
            feat = x['feat'].clone().requires_grad_()
            hpre = feat @ par['fc_w'].T + par['fc_b']
            h = torch.relu(hpre)
            if wrong == 'no_relu_mask':
                h = hpre + (h - hpre).detach()
            zmu = h @ par['mu_w'].T + par['mu_b']
            zls = h @ par['ls_w'].T + par['ls_b']
            for t in (hpre, zmu, zls):
                t.retain_grad()
            nodes.update(feat=feat, hpre=hpre)
            out['hpre'], out['zmu'][:ne], out['zls'][:ne] = hpre.detach() * we[:, None], zmu.detach() * we[:, None], \
                zls.detach() * we[:, None]
        else:
            zmu, zls = x['zmu'][:ne].clone().requires_grad_(), x['zls'][:ne].clone().requires_grad_()
        nodes.update(zmu=zmu, zls=zls)
        if f1 & REPARAM:
            z_e = zmu + torch.exp(zls) * x['eps_z'][:ne]
            terms['kl_enc'] = (we * kl_rows(zmu, zls)).sum()
            J = J + c.scales['kl_enc'] * terms['kl_enc']
            out['z'][:ne] = z_e.detach() * we[:, None]
        else:
            z_e = x['z'][:ne] + (zmu - zmu.detach())
            J = J + (we[:, None] * x['dzls'][:ne] * zls).sum()
        zs.append(z_e)
    # ---- the two variational segments
    segs = [(f1, nq, 0, '', c.scales['kl_q'], c.scales['lx'], ('kl_q', 'logl_x', 'ent')),
            (f2, nq2, nq, '2', c.scales['kl_q2'], c.scales['lx2'], ('kl_q2', 'logl_x2', 'ent2'))]
    gp_nodes = []
    for k, (fl, n, r0, sfx, kls, lxs, tn) in enumerate(segs):
        if n == 0:
            continue
        if k == 1 and wrong == 'seg2_scales':
            kls, lxs = segs[0][4], segs[0][5]
        if k == 1 and wrong == 'holdoff_gp':
            fl |= GP | (f1 & LOCKX)
        if k == 1 and wrong == 'seg2_rows':
            row = torch.arange(n) % nq
            pm = lambda name: par[name][row]
        else:
            pm = lambda name: par[name + sfx]
        rows, wq = slice(ne + r0, ne + r0 + n), w[ne + r0:ne + r0 + n]
        if fl & QZ:
            mu, ls = pm('qz_mu'), pm('qz_ls')
            z_q = mu + torch.exp(ls) * x['eps_z'][rows]
            terms[tn[0]] = (wq * kl_rows(mu, ls)).sum()
            J = J + kls * terms[tn[0]]
            out['z'][rows] = z_q.detach() * wq[:, None]
        else:
            z_q = x['z'][rows]
        zs.append(z_q)
        if fl & GP:
            qr = slice(r0, r0 + n)
            mux = z_q @ par['gp_w'].T + par['gp_b']
            mux.retain_grad()
            gp_nodes.append((qr, mux))
            if fl & LOCKX:
                xs = mux
            else:
                qls, gls = pm('qx_ls'), par['gp_ls']
                xs = pm('qx_mu') + torch.exp(qls) * x['eps_x'][qr]
                logl = (-0.5 * (2 * gls + ((xs - mux) / torch.exp(gls)) ** 2 + LOG2PI)).sum(1)
                terms[tn[1]] = (wq * logl).sum()
                terms[tn[2]] = (wq * qls.sum(1)).sum()
                J = J - lxs * (terms[tn[1]] + (0 if wrong == 'no_entropy' else terms[tn[2]]))
            J = J + (wq[:, None] * x['gxs'][qr] * xs).sum()
            out['mux'][qr], out['xs'][qr] = mux.detach() * wq[:, None], xs.detach() * wq[:, None]
    z = torch.cat(zs)
    if f1 & LATENT:
        lat = z @ par['lat_w'].T + par['lat_b']
        J = J + (w[:, None] * x['glat'] * lat).sum()
        out['lat'] = lat.detach() * w[:, None]
    else:
        J = J + (w[:, None] * x['gz'] * z).sum()
    J.backward()
    g = lambda t: torch.zeros_like(t) if t.grad is None else t.grad
    if ne:
        out['dzmu'][:ne], out['dzls'][:ne] = g(nodes['zmu']), g(nodes['zls'])
        if f1 & ENC:
            out['dhpre'], out['gfeat'] = g(nodes['hpre']), g(nodes['feat'])
    for qr, mux in gp_nodes:
        out['gmux'][qr] = g(mux)
    res = {k: v.double().numpy() for k, v in out.items()}
    res['terms'] = np.array([float(terms[k].detach()) for k in TERMS])
    for k, p in par.items():
        res['grad:' + k] = g(p).double().numpy()
    return res


def gemm_reference(items, ws):
    """A bare gpi_outer_gemm item list on the fp32 workspace array ws: per item (C [M, N], bias [M] or None) in
    fp64.  items: dicts with a_off, b_off, S, M, N, lda, ldb, relu, bias."""
    res = []
    w64 = np.asarray(ws, dtype=np.float64)
    for it in items:
        S, M, N = it['S'], it['M'], it['N']
        A = np.stack([w64[it['a_off'] + s * it['lda']:it['a_off'] + s * it['lda'] + M] for s in range(S)])
        Bm = np.stack([w64[it['b_off'] + s * it['ldb']:it['b_off'] + s * it['ldb'] + N] for s in range(S)])
        if it['relu']:
            Bm = np.maximum(Bm, 0.0)
        res.append((A.T @ Bm, A.sum(0) if it['bias'] else None))
    return res


def rel_err(a, r, same_rows=False):
    """The project's max|a - r| / max|r| over the entries the reference defines (not NaN).  A reference that is
    identically zero there must be met exactly (inf otherwise), a NaN in `a` where the reference has a value is inf;
    same_rows: `a` must be NaN exactly where the reference is (two references compared)."""
    a, r = np.asarray(a, dtype=np.float64), np.asarray(r, dtype=np.float64)
    m = ~np.isnan(r)
    if same_rows and (np.isnan(a) != ~m).any():
        return float('inf')
    if not m.any():
        return 0.0
    a, r = a[m], r[m]
    if np.isnan(a).any():
        return float('inf')
    d, den = np.abs(a - r).max(), np.abs(r).max()
    if den == 0:
        return 0.0 if d == 0 else float('inf')
    return float(d / den)
