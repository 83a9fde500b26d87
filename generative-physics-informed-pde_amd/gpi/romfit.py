"""Optimal effective properties: the batched ROM fit of gpi_rom_fit (csrc/rom.hip).

fit_effective_properties() runs every Adam iteration of the reference's OptimizeEffectiveProperties
(bottleneck/utils.py:250-282) for every labelled sample in ONE launch: the fit of
J = MSELoss(forward_mean(x, F), Y) over x, one wave per sample, the fine grid read once
(|W u - Y|^2 = u^T G u - 2 b^T u + c with G = W^T W, b = W^T Y, c = |Y|^2 in fp64).  No host
synchronisation here; the records stay on the device until the caller reads them.

Coarse meshes: nc = 4, 8 and 16 (rom_fit_kernel<NC>; nc = 16: the band factor and three sweeps per
iteration).  Any other nc raises NativeError (GPI_ERR_UNSUPPORTED); nothing falls back to a host loop here.
"""
import ctypes as C

import torch

from . import _lib as L

SUPPORTED_NC = (4, 8, 16)


class RomFitState(object):
    """Adam state of a fit (first / second moments [N, 2 nc^2] and the steps taken), to continue it."""

    def __init__(self, m, v, step):
        self.m, self.v, self.step = m, v, int(step)


class RomFitResult(object):
    """x        [N, 2 nc^2]  fitted log effective properties (after the last update)
    x_eval   [N, 2 nc^2]  the x the last iteration evaluated (the reference returns that prediction)
    uc       [N, (nc+1)^2] coarse solution at x_eval
    sumsq    [T, N] fp64  |W u(x) - Y_n|^2 at every evaluation (with y_weight: over the observed entries)
    ynorm2   [N] fp64     |Y_n|^2 (likewise)
    n_obs    the mean's denominator: n_total d_y, or the observed entries of the whole batch
    state    RomFitState  to continue the fit
    flag     int32 [1]    non-zero when a sample met kappa <= 1e-12 or a non-finite residual"""

    def __init__(self, x, x_eval, uc, sumsq, ynorm2, state, flag, n_total, d_y, n_obs=None):
        self.x, self.x_eval, self.uc, self.sumsq, self.ynorm2 = x, x_eval, uc, sumsq, ynorm2
        self.state, self.flag, self.n_total, self.d_y = state, flag, n_total, d_y
        self.n_obs = float(n_total * d_y) if n_obs is None else float(n_obs)

    def objective(self):
        """[T] fp64: the MSE of every evaluation, sum_n sumsq[t, n] / (n_total d_y) -- with y_weight
        / n_obs, the mean over the observed entries (torch's row reduction: a fixed order for a given shape,
        no atomics)."""
        return self.sumsq.sum(1) / self.n_obs

    def relerr(self, n):
        """relative_error_batched of evaluation n: mean_s sqrt(sumsq[n, s] / ynorm2[s]) (with y_weight both
        norms are over the sample's observed entries)."""
        return torch.mean(torch.sqrt(torch.clamp(self.sumsq[n], min=0.0) / self.ynorm2)).item()

    def check(self):
        """Raise if a sample's fit broke down (one host read of the flag)."""
        if int(self.flag.item()):
            raise L.NativeError('gpi_rom_fit: a sample met kappa <= 1e-12 or a non-finite residual')
        return self


def fit_effective_properties(Y, F, nc, refine, num_iterations, lr=1e-2, betas=(0.9, 0.999), eps=1e-8, x0=None,
                             state=None, n_total=None, y_weight=None, n_obs=None):
    """num_iterations Adam steps on x [N, 2 nc^2] (from x0, or zeros) against the labels Y [N, d_y] with
    the ROM right-hand sides F [N, (nc+1)^2].  state continues an earlier fit of the same rows; n_total is
    the N of the MSE mean (default: Y's rows; give the full count when fitting a part of a batch).
    nc in SUPPORTED_NC (4, 8, 16).

    y_weight: 0/1 observation weights of the label entries -- a bottleneck.utils.ObservedDofs, one shared
    row [d_y], or rows [N, d_y] (float or bool).  The objective is then the mean of the squared residual over
    the observed entries, and Y is never read into it where the weight is 0 (it may hold NaN there).
    n_obs is that mean's denominator, the observed entries of the WHOLE batch.  Default: n_total |index| for
    an ObservedDofs, with no host read; for a tensor ONE host read, y_weight.sum().item() (times n_total for
    a shared row) -- pass n_obs to avoid it, and always when the rows are a part of a batch with per-sample
    weights."""
    for t in (Y, F):
        L.require_device(t)
    nc, refine, T = int(nc), int(refine), int(num_iterations)
    N, nt, nn = Y.shape[0], 2 * nc * nc, (nc + 1) ** 2
    nf = nc * refine
    d_y = (nf + 1) * (nf - 1)
    if nc in SUPPORTED_NC and (tuple(Y.shape) != (N, d_y) or tuple(F.shape) != (N, nn)):
        raise ValueError('Y %s / F %s do not match nc = %d, refine = %d' % (tuple(Y.shape), tuple(F.shape), nc, refine))
    dev = Y.device
    Y, F = Y.contiguous().float(), F.contiguous().float()
    nt_all = N if n_total is None else int(n_total)
    yw = None
    if y_weight is not None:
        if not torch.is_tensor(y_weight):          # an ObservedDofs: its cached row, its count
            if n_obs is None:
                n_obs = float(nt_all) * len(y_weight.index)
            yw = y_weight.weights(d_y, dev)
        else:
            L.require_device(y_weight)
            if tuple(y_weight.shape) not in ((d_y,), (N, d_y)):
                raise ValueError('y_weight %s is neither [%d] nor [%d, %d]' % (tuple(y_weight.shape), d_y, N, d_y))
            yw = y_weight.to(torch.float32).contiguous()
            if n_obs is None:
                n_obs = float(yw.sum(dtype=torch.float64).item()) * (nt_all if yw.dim() == 1 else 1)
        if not n_obs > 0:
            raise ValueError('y_weight observes no label entry (n_obs = %r)' % (n_obs,))
    elif n_obs is not None:
        raise ValueError('n_obs without y_weight')
    x = torch.zeros(N, nt, device=dev) if x0 is None else x0.detach().to(dev, torch.float32).clone().contiguous()
    if state is None:
        m, v, step0 = torch.zeros(N, nt, device=dev), torch.zeros(N, nt, device=dev), 0
    else:
        m, v, step0 = state.m.clone().contiguous(), state.v.clone().contiguous(), state.step
    x_eval = x.clone()
    uc = torch.zeros(N, nn, device=dev)
    sumsq = torch.zeros(T, N, dtype=torch.float64, device=dev)
    ynorm2 = torch.zeros(N, dtype=torch.float64, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    d = L.RomFitDesc()
    d.nc, d.refine, d.n, d.iters = nc, refine, N, T
    d.n_total = nt_all
    if yw is not None:
        d.y_weight, d.yw_stride, d.n_obs = yw.data_ptr(), (d_y if yw.dim() == 2 else 0), float(n_obs)
    d.Y, d.F, d.x, d.x_stride = Y.data_ptr(), F.data_ptr(), x.data_ptr(), x.stride(0) if N else nt
    d.m, d.v, d.step0 = m.data_ptr(), v.data_ptr(), step0
    d.lr, d.beta1, d.beta2, d.eps = lr, betas[0], betas[1], eps
    d.sumsq, d.ynorm2, d.x_eval, d.uc, d.flag = (sumsq.data_ptr(), ynorm2.data_ptr(), x_eval.data_ptr(),
                                                 uc.data_ptr(), flag.data_ptr())
    L.check(L.lib().gpi_rom_fit(C.byref(d), L.stream_handle()), 'rom fit')
    return RomFitResult(x, x_eval, uc, sumsq, ynorm2, RomFitState(m, v, step0 + T), flag, d.n_total or N, d_y,
                        n_obs=n_obs)
