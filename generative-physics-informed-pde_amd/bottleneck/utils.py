"""Gaussian helpers and the optimal-effective-property fit (reference bottleneck/utils.py:216-282).

Tensor-level utilities kept with the reference's names and signatures for
callers outside the fused step (e.g. monitoring); the training step computes
the same quantities inside the native kernels (head.hip, conv.hip, rom.hip).
OptimizeEffectiveProperties runs on gpi_rom_fit (gpi/romfit.py).
"""
import torch

LOG2PI = 1.8378770664093453


def reparametrize(mean, logsigma):
    return mean + torch.exp(logsigma) * torch.randn_like(logsigma)


def DiagonalGaussianLogLikelihood(target, mean, logvars, target_logvars=None, reduce=torch.sum):
    if target_logvars is not None:
        raise DeprecationWarning
    L = -0.5 * (logvars + (target - mean) ** 2 * torch.exp(-logvars) + LOG2PI)
    return reduce(L) if reduce is not None else L


def UnitGaussianKullbackLeiblerDivergence(mean, logvars):
    return -0.5 * torch.sum(1 + logvars - mean.pow(2) - logvars.exp())


def relative_error(y, y_true):
    return (torch.norm(y - y_true) / torch.norm(y_true)).item()


def relative_error_batched(Y_mean, Y_true):
    return torch.mean(torch.norm(Y_mean - Y_true, dim=1) / torch.norm(Y_true, dim=1)).item()


class ObservedDofs(object):
    """Partially observed labels: the PDE solution known at the fine free nodes ``index`` (sensors).

    As a callable it is the reference's column-selecting hook, ``y -> y[..., index]``
    (GenerativeModel.preprocess_y_fct, OptimizeEffectiveProperties' y_preprocessor), so reference-style
    callers and the module-path loops work with it.  The native kernels take the same set as a 0/1
    observation weight per label entry (gpi_rom_desc.y_weight): ``weights(d_y, device)``."""

    def __init__(self, index):
        index = torch.as_tensor(index, dtype=torch.long).reshape(-1).cpu()
        if index.numel() and int(index.min()) < 0:
            raise ValueError('ObservedDofs: negative node index')
        if index.unique().numel() != index.numel():
            raise ValueError('ObservedDofs: the node indices must be distinct (each is one observed entry)')
        self.index = index
        self._weights = {}
        self._dev_index = {}

    def __len__(self):
        return self.index.numel()

    def __call__(self, y):
        dev = y.device
        idx = self._dev_index.get(dev)
        if idx is None:
            idx = self._dev_index[dev] = self.index.to(dev)
        return y[..., idx]

    def weights(self, d_y, device):
        """The fp32 row [d_y], 1 at the observed nodes and 0 elsewhere (one tensor per (d_y, device), kept:
        its address is what launch descriptors and captured graphs hold)."""
        key = (int(d_y), torch.device(device))
        w = self._weights.get(key)
        if w is None:
            if self.index.numel() and int(self.index.max()) >= d_y:
                raise ValueError('ObservedDofs: node index %d outside the %d label entries' % (int(self.index.max()), d_y))
            w = torch.zeros(int(d_y), dtype=torch.float32)
            w[self.index] = 1.0
            w = self._weights[key] = w.to(device)
        return w


def OptimizeEffectiveProperties(dataset, g, num_iterations=300, lr=1e-2, verbose=True, y_preprocessor=None):
    """The log effective properties that best reproduce the labels through the ROM g (reference
    bottleneck/utils.py:250-282): Adam from logX = 0 on MSELoss(g.forward_mean(logX, F_ROM_BC), Y) over
    every labelled sample.  Returns (logX_effprop, Y_predict, objective, relerr_list): the fitted rows,
    the prediction of the last iteration (before its update), the objective of every iteration and the
    batched relative error at iterations 100, 200, ... (of the prediction made one iteration earlier).

    nc = 4 / 8 / 16 without a y_preprocessor, or with an ObservedDofs (labels at sensor nodes: the objective
    over the observed entries, Y_predict column-selected as the reference returns it): one gpi_rom_fit launch
    (gpi/romfit.py).  Any other y_preprocessor: the same loop through g.forward_mean (gpi_rom) and
    torch.optim.Adam on the device."""
    Y = dataset.get('Y')
    F_ROM_BC = dataset.get('F_ROM_BC')
    rom = getattr(g, 'rom', None)
    observed = y_preprocessor if isinstance(y_preprocessor, ObservedDofs) else None
    if (y_preprocessor is None or observed is not None) and rom is not None and Y.shape[0] > 0:
        from gpi import romfit
        if rom.nc in romfit.SUPPORTED_NC:
            yw = observed.weights(Y.shape[1], Y.device) if observed is not None else None
            fit = romfit.fit_effective_properties(Y, F_ROM_BC, rom.nc, rom.refine, num_iterations, lr=lr,
                                                  y_weight=yw).check()
            relerr_list = [fit.relerr(n - 1) for n in range(100, num_iterations, 100)]
            if verbose:
                for k, e in enumerate(relerr_list):
                    print("Iteration {} || RelErr : {}".format(100 * (k + 1), e))
            if num_iterations > 0:
                Y_predict = g.forward_mean(fit.x_eval, F_ROM_BC).detach()
                if observed is not None:
                    Y_predict = observed(Y_predict)
            else:
                Y_predict = None
            logX_effprop = fit.x.to(Y.dtype).requires_grad_(True)
            return logX_effprop, Y_predict, fit.objective().tolist(), relerr_list

    if y_preprocessor is not None:
        Y = y_preprocessor(Y)
    logX_effprop = torch.zeros(Y.shape[0], g.dim_effective_property, dtype=Y.dtype, device=Y.device,
                               requires_grad=True)
    optimizer = torch.optim.Adam([logX_effprop], lr=lr)
    loss = torch.nn.MSELoss()
    objective, relerr_list = [], []
    Y_predict = None
    for n in range(num_iterations):
        if n % 100 == 0 and n > 0:
            with torch.no_grad():
                myrelerr = relative_error_batched(Y_predict, Y)
                relerr_list.append(myrelerr)
            if verbose:
                print("Iteration {} || RelErr : {}".format(n, myrelerr))
        Y_predict = g.forward_mean(logX_effprop, F_ROM_BC)
        if y_preprocessor is not None:
            Y_predict = y_preprocessor(Y_predict)
        J = loss(Y_predict, Y)
        optimizer.zero_grad()
        J.backward()
        objective.append(J.item())
        optimizer.step()
    return logX_effprop, Y_predict, objective, relerr_list
