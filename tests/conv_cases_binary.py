"""The Bernoulli-loss rows of the per-operator conv sweep (tests/test_gpu_binary_conv.py): the four
Gaussian-loss rows of tests/conv_cases.py with cout = 1 and the GPI_EPI_BERNOULLI_LOSS epilogue -- the smallest
shapes that reach each tile form of the 5x5 output conv -- in the same producer / T chain, built here because
conv_cases.chain() gives its loss op a two-channel output.  Targets are two-valued; `lo` / `hi` give each BN
group's phase values (row 3: the two groups have different low-phase values)."""
import numpy as np
import torch

from gpi import _lib as L
from gpi.plan import CodecProgram
from conv_cases import Case, CASES as GAUSS_CASES

LOGIT_MAX = 15.0


def B_(cin, h, groups, seed, lo, hi, **kw):
    c = Case(5, 's1', cin, 1, h, h, groups, loss='bern', seed=seed, **kw)
    c.lo, c.hi = list(lo), list(hi)
    return c


LOG1, LOG10 = float(np.log(1.0)), float(np.log(10.0))
CASES = [
    B_(3, 16, [2, 1], 134, [LOG1, LOG1], [LOG10, LOG10]),
    B_(1, 8, [2], 135, [LOG1], [LOG10]),
    B_(4, 32, [32, 8], 136, [LOG1, -0.5], [LOG10, 1.25]),          # x_lo differs between the groups
    B_(4, 64, [64, 8], 137, [LOG1, LOG1], [LOG10, LOG10], shuffle=True, loss_scale=[0.5, 1.0 / 8]),
]


def gauss_twin(case):
    """The Gaussian-loss row of conv_cases.py this row mirrors (same cin, plane, groups)."""
    tw = [c for c in GAUSS_CASES if c.loss and (c.cin, c.h, c.w, c.groups) == (case.cin, case.h, case.w, case.groups)]
    assert len(tw) == 1, case.id
    return tw[0]


def chain(case):
    """z (4 channels) -> 1x1 producers -> X (cin) -> T: BN + ReLU + 5x5 conv -> one logit channel, Bernoulli
    epilogue; T's output buffer is the program's output."""
    P = CodecProgram('decoder', 0.0)
    h, w = case.h, case.w
    z = P.buf('z', 4, h, w)
    P.input = z
    X = P.buf('X', case.cin, h, w)
    Y = P.buf('out', 1, h, w)
    for i, c0 in enumerate(range(0, case.cin, L.GPI_MAX_COUT)):
        n = min(L.GPI_MAX_COUT, case.cin - c0)
        P.conv('p%d' % i, z, 0, 4, X, c0, n, 1, 1, 0, 0, 'p%d.weight' % i)
    P.T = P.conv('T', X, 0, case.cin, Y, 0, 1, 5, 1, 2, 0, 'T.weight', bn='T.bn', epilogue=L.EPI_BERNOULLI_LOSS)
    P.output = Y
    return P


def two_valued_targets(case, targets, seed):
    """Replace the Gaussian rows' random targets by two-valued ones of the same shapes: each group's rows hold
    its lo / hi values, both present, the group's minimum = lo."""
    gen = torch.Generator().manual_seed(2000 + seed)
    out = []
    for g, t in enumerate(targets):
        bits = torch.rand(t.shape, generator=gen) < 0.45
        bits.view(-1)[0], bits.view(-1)[1] = False, True
        out.append(torch.where(bits, torch.tensor(case.hi[g]), torch.tensor(case.lo[g])).float())
        assert float(out[-1].min()) == np.float32(case.lo[g])
    return out


def softplus(v):
    return torch.clamp(v, min=0) + torch.log1p(torch.exp(-v.abs()))


def bernoulli_terms(a, targets, target_idx, groups, lows, loss_scale):
    """(per-group log-likelihoods [groups], objective -sum_g scale_g logl_g) of the logit image a [B, 1, H, W]
    against the target bits t = (target != lows[g]), in a's dtype."""
    logl, s = [], 0
    for g, n in enumerate(groups):
        t = targets[g].reshape(-1, a.shape[2], a.shape[3])
        if target_idx is not None and target_idx[g] is not None:
            t = t[torch.as_tensor(target_idx[g], dtype=torch.long)]
        bit = t[:n] != np.float32(lows[g])
        ag = a[s:s + n, 0]
        logl.append(-torch.where(bit, softplus(-ag), softplus(ag)).sum())
        s += n
    logl = torch.stack(logl)
    scale = torch.as_tensor(loss_scale, dtype=a.dtype)
    return logl, -(scale * logl).sum()
