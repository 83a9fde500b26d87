"""The homoscedastic-Gaussian-loss rows of the per-operator conv sweep (tests/test_gpu_homosc_conv.py): the four
Gaussian-loss rows of tests/conv_cases.py with cout = 1 and the GPI_EPI_GAUSS_HOMO_LOSS / GPI_EPI_GAUSS_HOMO_EXP_LOSS
epilogues -- the smallest shapes that reach each tile form of the 5x5 output conv (8^2 and 16^2: one tile per
sample; 32^2: 8-row forward tiles; 64^2: several tiles per sample, half tiles, so halo rows overlap in the fused
recompute) -- in the same producer / T chain, built here because conv_cases.chain() gives its loss op a
two-channel output.  Each row runs with both epilogues.  The learned log-sigma plane is the extra parameter
'T.logsigma' [H, W]; its per-sample gradient rows [B][H W] follow the ops' slabs in the partial-slab arena."""
import math

import torch

from gpi import _lib as L
from gpi.plan import CodecProgram
from conv_cases import Case, CASES as GAUSS_CASES, param_shapes as conv_param_shapes

LOG2PI = math.log(2.0 * math.pi)
PLANE = 'T.logsigma'


def H_(cin, h, groups, seed, exp_field, **kw):
    c = Case(5, 's1', cin, 1, h, h, groups, loss='homoexp' if exp_field else 'homo', seed=seed, **kw)
    c.exp_field = bool(exp_field)
    return c


def _rows(exp_field, seed0):
    return [
        H_(3, 16, [2, 1], seed0, exp_field),
        H_(1, 8, [2], seed0 + 1, exp_field),
        H_(4, 32, [32, 8], seed0 + 2, exp_field),
        H_(4, 64, [64, 8], seed0 + 3, exp_field, shuffle=True, loss_scale=[0.5, 1.0 / 8]),
    ]


CASES = _rows(False, 234) + _rows(True, 244)


def epilogue_of(case):
    return L.EPI_GAUSS_HOMO_EXP_LOSS if case.exp_field else L.EPI_GAUSS_HOMO_LOSS


def gauss_twin(case):
    """The Gaussian-loss row of conv_cases.py this row mirrors (same cin, plane, groups)."""
    tw = [c for c in GAUSS_CASES if c.loss and (c.cin, c.h, c.w, c.groups) == (case.cin, case.h, case.w, case.groups)]
    assert len(tw) == 1, case.id
    return tw[0]


def chain(case):
    """z (4 channels) -> 1x1 producers -> X (cin) -> T: BN + ReLU + 5x5 conv -> one mean channel, homoscedastic
    epilogue; T's output buffer is the program's output.  prog.gls_off: the per-sample d/d(log sigma) rows'
    offset in the partial-slab arena, set by lay_out_with_rows()."""
    P = CodecProgram('decoder', 0.0)
    h, w = case.h, case.w
    z = P.buf('z', 4, h, w)
    P.input = z
    X = P.buf('X', case.cin, h, w)
    Y = P.buf('out', 1, h, w)
    for i, c0 in enumerate(range(0, case.cin, L.GPI_MAX_COUT)):
        n = min(L.GPI_MAX_COUT, case.cin - c0)
        P.conv('p%d' % i, z, 0, 4, X, c0, n, 1, 1, 0, 0, 'p%d.weight' % i)
    P.T = P.conv('T', X, 0, case.cin, Y, 0, 1, 5, 1, 2, 0, 'T.weight', bn='T.bn', epilogue=epilogue_of(case))
    P.output = Y
    P.gls_off = None
    return P


def param_shapes(prog):
    """conv_cases.param_shapes plus the plane (a matrix parameter: FlatParameters starts it on a 16-byte boundary)."""
    return conv_param_shapes(prog) + [(PLANE, (prog.output.H, prog.output.W))]


def plane_reduce_item(prog, B, param_offset):
    """The cross-batch sum of the per-sample rows: one more gpi_reduce_item (blocks = B, numel = row_stride = H W)."""
    it = L.ReduceItem()
    hw = prog.output.H * prog.output.W
    it.part_off, it.w_off, it.numel, it.row_stride, it.blocks = prog.gls_off, param_offset(PLANE), hw, hw, B
    return it


def homosc_terms(mean, plane, targets, target_idx, groups, exp_field, loss_scale):
    """(per-group log-likelihoods [groups], objective -sum_g scale_g logl_g, per-sample d(objective)/d(log sigma)
    rows [B, H W]) of the mean image [B, 1, H, W] against the targets with log sigma = plane [H, W], in mean's
    dtype: ll = -1/2 (2 ls + r^2 exp(-2 ls) + log 2 pi), r = t - mean or exp(t) - exp(mean)."""
    logl, rows, s = [], [], 0
    scale = torch.as_tensor(loss_scale, dtype=mean.dtype)
    e = torch.exp(-2.0 * plane)
    for g, n in enumerate(groups):
        t = targets[g].to(mean.dtype).reshape(-1, mean.shape[2], mean.shape[3])
        if target_idx is not None and target_idx[g] is not None:
            t = t[torch.as_tensor(target_idx[g], dtype=torch.long)]
        m = mean[s:s + n, 0]
        r = (torch.exp(t[:n]) - torch.exp(m)) if exp_field else (t[:n] - m)
        logl.append((-0.5 * (2.0 * plane + r * r * e + LOG2PI)).sum())
        rows.append((scale[g] * (1.0 - r * r * e)).detach().reshape(n, -1))
        s += n
    logl = torch.stack(logl)
    return logl, -(scale * logl).sum(), torch.cat(rows, 0)
