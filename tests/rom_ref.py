"""Plain torch reference of the coarse-grained model operator (gpi_rom), fp64 on the CPU, one function per mode.

Built on oracle/elbo.py (rom_solve: the reference's dense K = M x^T, the Dirichlet rows replaced by identity rows,
a dense batched solve; dgll: DiagonalGaussianLogLikelihood) and on elbo_ref.physics(nc, r) (M and the dense P1
prolongation W from the generic finite-element restatement, oracle/fem.py).  Every gradient is autograd's.

    forward   uc = K(kappa)^{-1} F,  mu = W uc                      ROM.py:65-100, components.py:296-298
    loglik    L = sum -1/2 (2 ls + ((Y - mu) / exp(ls))^2 + log 2 pi)   bottleneck/utils.py:231-243
              gx = loss_scale d(-L)/dx,  gls = loss_scale d(-L)/dlogsigma_y (per-sample rows and their sum);
              loss_scale multiplies the gradients and not the value
    backward  gx = d/dx of J = <dmu, W uc> + <duc, uc>
kappa = exp(x) + 1e-8, or x itself with input_kappa (the gradients are then d/dkappa).

`wrong` selects a deliberately wrong variant (tests/test_rom_cases_plan.py: what the comparison must notice);
`dtype` the evaluation precision (float32: the attainability check of the bars).
"""
import numpy as np
import torch

from elbo_ref import physics
from oracle import elbo as oelbo
from oracle import fem

WRONG = ('backslash', 'rows_r', 'no_duc', 'kappa_eps', 'no_lift', 'scale_value')
_T = {}
_WB = {}


def tensors(nc, r, dtype=torch.float64):
    """(M, W, bc) of physics(nc, r) as torch tensors of `dtype`, kept."""
    key = (nc, r, dtype)
    if key not in _T:
        M, W, bc = physics(nc, r)
        _T[key] = (torch.tensor(M, dtype=dtype), torch.tensor(W, dtype=dtype), torch.as_tensor(bc))
    return _T[key]


def backslash_prolongation(nc, r):
    """W of a coarse mesh whose squares are split along the other diagonal (v1 - v2 instead of v0 - v3)."""
    key = (nc, r)
    if key not in _WB:
        mc, mf = fem.unit_square_mesh(nc), fem.unit_square_mesh(nc * r)
        cells = []
        for v0, v1, v3 in mc.cells[0::2]:
            v2 = v3 - 1
            cells += [(v0, v1, v2), (v1, v3, v2)]
        _WB[key] = fem.prolongation_free(fem.TriMesh(mc.coords, cells), mf)
    return _WB[key]


def _W(nc, r, dtype, wrong):
    W = tensors(nc, r, dtype)[1]
    if wrong == 'backslash':
        W = torch.tensor(backslash_prolongation(nc, r), dtype=dtype)
    if wrong == 'rows_r':                       # the fine row y = 1 (the last n - 1 free nodes) is never visited
        W = W.clone()
        W[-(nc * r - 1):] = 0
    return W


def _solve(nc, r, x, F, input_kappa, dtype, wrong):
    """x: a leaf tensor [N, 2 nc^2] -> uc [N, (nc + 1)^2]"""
    M, _, bc = tensors(nc, r, dtype)
    if input_kappa:
        kappa = x + 1e-8 if wrong == 'kappa_eps' else x
    else:
        kappa = torch.exp(x) + 1e-8
    if wrong != 'no_lift':
        return oelbo.rom_solve(M, kappa, F, bc)
    # rhs of the interior rows without - K_IB F_B: the Dirichlet columns of K dropped from the interior rows
    if (kappa <= 1e-12).any():
        raise ValueError('kappa <= 1e-12')
    K = torch.matmul(M, kappa.t())
    K[:, bc] = 0
    K[bc] = 0
    K[bc, bc] = 1
    return torch.linalg.solve(K.permute(2, 0, 1), F.unsqueeze(2)).squeeze(2)


def _prep(a, dtype, grad=False):
    return torch.tensor(np.asarray(a, dtype=np.float64), dtype=dtype, requires_grad=grad)


def _np(t):
    return t.detach().double().numpy()


def forward(nc, r, x, F, input_kappa=False, dtype=torch.float64, wrong=None):
    """-> dict(uc [N, nn], mu [N, dy])"""
    assert wrong is None or wrong in WRONG
    uc = _solve(nc, r, _prep(x, dtype), _prep(F, dtype), input_kappa, dtype, wrong)
    mu = torch.einsum('sk,nk->ns', _W(nc, r, dtype, wrong), uc)
    return dict(uc=_np(uc), mu=_np(mu))


def loglik(nc, r, x, F, Y, ls, loss_scale=1.0, input_kappa=False, dtype=torch.float64, wrong=None):
    """-> dict(uc, mu, L (float), L_rows [N], gx [N, nT], gls [dy], gls_rows [N, dy])"""
    assert wrong is None or wrong in WRONG
    N = np.asarray(x).shape[0]
    xt = _prep(x, dtype, True)
    lsr = _prep(ls, dtype).repeat(N, 1).requires_grad_()          # one row per sample: per-sample d/dlogsigma_y
    uc = _solve(nc, r, xt, _prep(F, dtype), input_kappa, dtype, wrong)
    mu = torch.einsum('sk,nk->ns', _W(nc, r, dtype, wrong), uc)
    Yt = _prep(Y, dtype)
    rows = torch.stack([oelbo.dgll(Yt[s], mu[s], 2 * lsr[s]) for s in range(N)])
    L = rows.sum()
    (-loss_scale * L).backward()
    val = L * loss_scale if wrong == 'scale_value' else L
    rows_v = rows * loss_scale if wrong == 'scale_value' else rows
    return dict(uc=_np(uc), mu=_np(mu), L=float(val.detach()), L_rows=_np(rows_v), gx=_np(xt.grad),
                gls=_np(lsr.grad.sum(0)), gls_rows=_np(lsr.grad))


def backward(nc, r, x, F, dmu=None, duc=None, input_kappa=False, dtype=torch.float64, wrong=None):
    """-> dict(gx [N, nT]): d/dx (d/dkappa with input_kappa) of J = <dmu, W uc> + <duc, uc>"""
    assert wrong is None or wrong in WRONG
    assert dmu is not None or duc is not None
    xt = _prep(x, dtype, True)
    uc = _solve(nc, r, xt, _prep(F, dtype), input_kappa, dtype, wrong)
    J = 0
    if dmu is not None:
        J = J + (_prep(dmu, dtype) * torch.einsum('sk,nk->ns', _W(nc, r, dtype, wrong), uc)).sum()
    if duc is not None and not (wrong == 'no_duc' and dmu is not None):
        J = J + (_prep(duc, dtype) * uc).sum()
    J.backward()
    return dict(gx=_np(xt.grad))


def rel_err(a, ref):
    """The project's tensor_rel, max|a - ref| / max|ref|; a NaN in `a` is inf."""
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if np.isnan(a).any():
        return float('inf')
    return float(np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-300))
