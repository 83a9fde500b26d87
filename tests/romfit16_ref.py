"""romfit_ref.fit with the stiffness tensor held sparse, for the 16 x 16 coarse mesh: the dense
[289, 289, 512] contraction K = M kappa^T costs about a second per iteration and sample there, the
sparse one ([289^2, 512] with <= 4 entries per row of K) next to nothing.  The same loop otherwise:
Dirichlet rows as oracle.elbo.rom_solve, torch.linalg.solve, mse_loss, torch.optim.Adam from x = 0, any
dtype (fp64: the yardstick of tests/test_gpu_romfit16.py; fp32: what a fp32 path can hold at all)."""
import numpy as np
import torch

from elbo_ref import physics
from oracle import fem
from romfit_ref import MARKS, _t


def sparse_stiffness(M, dtype):
    """M [n, n, n_T] as a sparse [n^2, n_T] matrix."""
    M = np.asarray(M)
    n, _, nt = M.shape
    i, j, t = np.nonzero(M)
    idx = torch.as_tensor(np.stack([i * n + j, t]), dtype=torch.long)
    return torch.sparse_coo_tensor(idx, _t(M[i, j, t], dtype), (n * n, nt)).coalesce()


def rom_solve(Msp, n, kappa, F, bc):
    """oracle.elbo.rom_solve with K_n = (M_sp kappa_n) reshaped."""
    if (kappa <= 1e-12).any():
        raise ValueError('kappa <= 1e-12')
    K = torch.sparse.mm(Msp, kappa.t()).reshape(n, n, kappa.shape[0])
    K[bc] = 0
    K[bc, bc] = 1
    return torch.linalg.solve(K.permute(2, 0, 1), F.unsqueeze(2)).squeeze(2)


def synthetic_labels(nc, r, N, seed, noise):
    """Seeded fp32 (Y, F) for the (nc, r) ROM: Y = W u(x*) + noise randn, x* = 0.7 randn, F from random corner
    data (fp64, rounded to fp32 once: every implementation reads the same numbers)."""
    M, W, bc = physics(nc, r)
    rng = np.random.default_rng(seed)
    mc = fem.unit_square_mesh(nc)
    F = np.stack([fem.f_rom_bc(mc, u) for u in rng.uniform(-0.5, 0.5, (N, 4))]).astype(np.float32)
    xs = torch.tensor(0.7 * rng.standard_normal((N, M.shape[2])))
    u = rom_solve(sparse_stiffness(M, torch.float64), M.shape[0], torch.exp(xs) + 1e-8,
                  torch.tensor(F, dtype=torch.float64), torch.as_tensor(np.asarray(bc), dtype=torch.long))
    mu = u.numpy() @ np.asarray(W).T
    return (mu + noise * rng.standard_normal(mu.shape)).astype(np.float32), F


def fit(W, M, bc, Y, F, T, lr, dtype=torch.float64, marks=MARKS):
    """T Adam iterations; the dict of romfit_ref.fit."""
    n = np.asarray(M).shape[0]
    Msp = sparse_stiffness(M, dtype)
    W, Y, F = _t(W, dtype), _t(Y, dtype), _t(F, dtype)
    bc = torch.as_tensor(np.asarray(bc), dtype=torch.long)
    N, dy = Y.shape
    x = torch.zeros(N, Msp.shape[1], dtype=dtype, requires_grad=True)
    opt = torch.optim.Adam([x], lr=lr)
    ynorm2 = torch.sum(Y ** 2, 1)
    objective, sumsq, relerr_list, x_marks = [], [], [], {}
    x_eval = Y_predict = None
    for it in range(T):
        if it % 100 == 0 and it > 0:
            relerr_list.append(torch.mean(torch.sqrt(sumsq[-1]) / torch.sqrt(ynorm2)).item())
        x_eval = x.detach().clone()
        u = rom_solve(Msp, n, torch.exp(x) + 1e-8, F, bc)
        mu = torch.einsum('sk,nk->ns', W, u)
        J = torch.nn.functional.mse_loss(mu, Y)
        ss = torch.sum((mu - Y) ** 2, 1)
        Y_predict = mu.detach()
        opt.zero_grad()
        J.backward()
        objective.append(J.item())
        sumsq.append(ss.detach())
        opt.step()
        if it + 1 in marks:
            x_marks[it + 1] = x.detach().clone().numpy()
    return dict(x=x.detach().numpy(), x_marks=x_marks, x_eval=None if x_eval is None else x_eval.numpy(),
                Y_predict=None if Y_predict is None else Y_predict.numpy(),
                objective=np.asarray(objective, dtype=np.float64),
                sumsq=torch.stack(sumsq).numpy() if sumsq else np.zeros((0, N)), ynorm2=ynorm2.numpy(),
                relerr_list=relerr_list)
