"""Restatement of OptimizeEffectiveProperties (reference bottleneck/utils.py:250-282) for the tests:
oracle.elbo.rom_operator + torch.nn.functional.mse_loss + torch.optim.Adam from logX = 0, any dtype
(fp64: the yardstick of the GPU tests), in the reference's direct form and in the reduced form the
kernel uses (|W u - Y|^2 = u^T G u - 2 b^T u + c with G = W^T W, b = W^T Y, c = |Y|^2)."""
import numpy as np
import torch

from oracle import elbo as oelbo

MARKS = (1, 10, 50, 300)


def _t(a, dtype):
    return torch.as_tensor(np.asarray(a), dtype=dtype)


def fit(W, M, bc, Y, F, T, lr, dtype=torch.float64, reduced=False, marks=MARKS):
    """T Adam iterations.  Returns a dict of numpy arrays:
    x [N, d_x] after T updates, x_marks {n: x after n updates}, x_eval (before the last update),
    Y_predict (the last iteration's prediction), objective [T], sumsq [T, N], ynorm2 [N], relerr_list
    (at n = 100, 200, ..., of iteration n - 1's prediction, as the reference logs it)."""
    W, M, Y, F = _t(W, dtype), _t(M, dtype), _t(Y, dtype), _t(F, dtype)
    bc = torch.as_tensor(np.asarray(bc), dtype=torch.long)
    N, dy = Y.shape
    x = torch.zeros(N, M.shape[2], dtype=dtype, requires_grad=True)
    opt = torch.optim.Adam([x], lr=lr)
    ls = torch.zeros(dy, dtype=dtype)
    ynorm2 = torch.sum(Y ** 2, 1)
    if reduced:
        G, b = W.t() @ W, Y @ W
    objective, sumsq, relerr_list, x_marks = [], [], [], {}
    x_eval = Y_predict = None
    for n in range(T):
        if n % 100 == 0 and n > 0:
            relerr_list.append(torch.mean(torch.sqrt(sumsq[-1]) / torch.sqrt(ynorm2)).item())
        x_eval = x.detach().clone()
        if reduced:
            u = oelbo.rom_solve(M, torch.exp(x) + 1e-8, F, bc)
            ss = torch.einsum('ni,ij,nj->n', u, G, u) - 2 * torch.sum(b * u, 1) + ynorm2
            J = torch.sum(ss) / (N * dy)
            Y_predict = None
        else:
            mu, _ = oelbo.rom_operator(W, M, bc, x, F, ls)
            J = torch.nn.functional.mse_loss(mu, Y)
            ss = torch.sum((mu - Y) ** 2, 1)
            Y_predict = mu.detach()
        opt.zero_grad()
        J.backward()
        objective.append(J.item())
        sumsq.append(ss.detach())
        opt.step()
        if n + 1 in marks:
            x_marks[n + 1] = x.detach().clone().numpy()
    return dict(x=x.detach().numpy(), x_marks=x_marks, x_eval=None if x_eval is None else x_eval.numpy(),
                Y_predict=None if Y_predict is None else Y_predict.numpy(),
                objective=np.asarray(objective, dtype=np.float64),
                sumsq=torch.stack(sumsq).numpy() if sumsq else np.zeros((0, N)), ynorm2=ynorm2.numpy(),
                relerr_list=relerr_list)


def x_drift(x_marks, ref_marks):
    """max over the marks of max|x - ref| / max|ref|."""
    return max(float(np.abs(np.asarray(x_marks[n], dtype=np.float64) - ref_marks[n]).max() / np.abs(ref_marks[n]).max())
               for n in ref_marks)


def j_drift(objective, ref):
    """max relative deviation of the objective history."""
    objective, ref = np.asarray(objective, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.max(np.abs(objective - ref) / np.abs(ref)))
