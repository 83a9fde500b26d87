"""Test-only CPU interpreter of a planned codec program (gpi/plan.py).

Executes the op list with torch ops, reading each op's channel ranges,
BN parameter names and conv geometry exactly as the HIP kernels do, so the
planner's wiring (buffers, channel offsets, concat-in-place, BN placement)
is validated on CPU against the oracle codec.  Never used by the product.

evaluate() is the full form (the per-operator sweep's fp64 reference, tests/test_gpu_conv_ops.py):
differentiable, with given ReLU decisions, Dropout2d scales and the Gaussian-loss epilogues;
run_program() keeps the plain forward of the planner tests.
"""
import math

import torch
import torch.nn.functional as F

EPI_GAUSS_LOSS, EPI_GAUSS_EXP_LOSS = 2, 3      # include/gpi.h GPI_EPI_*
LOG2PI = math.log(2.0 * math.pi)


class Result(object):
    """bufs: buffer name -> final [B, C, H, W] tensor; output: the program's output buffer;
    logl: [groups] Gaussian log-likelihood sums of the loss op (None without one);
    objective: -sum_g loss_scale[g] logl[g] (None without a loss op);
    audit: [(bn name, decisions that differ from the interpreter's own bn(x) > 0, largest |bn(x)| among
    them, elements)] for every layer a mask was given for (the shape of oracle/codec.py's MASK_AUDIT)."""

    def __init__(self):
        self.bufs, self.output, self.logl, self.objective, self.audit = {}, None, None, None, []


def _bn(src, groups, gamma, beta):
    outs = []
    s = 0
    for n in groups:
        outs.append(F.batch_norm(src[s:s + n], None, None, gamma, beta, training=True, eps=1e-5))
        s += n
    return torch.cat(outs, 0)


def gauss_logl(y, t, exp_field):
    """sum -0.5 (2 ls + r^2 exp(-2 ls) + log 2 pi) over y = (mu, ls) [n, 2, H, W] against t [n, H, W]:
    r = t - mu, or exp(t) - exp(mu) for the exponentiated field (gpi.h GPI_EPI_GAUSS_EXP_LOSS)."""
    mu, ls = y[:, 0], y[:, 1]
    r = (torch.exp(t) - torch.exp(mu)) if exp_field else (t - mu)
    return (-0.5 * (2.0 * ls + r * r * torch.exp(-2.0 * ls) + LOG2PI)).sum()


def evaluate(prog, params, x, groups=None, masks=None, drops=None, targets=None, target_idx=None,
             loss_scale=None):
    """prog: CodecProgram; params: name -> tensor; x: input [B, C, H, W] (already gathered when the program's
    input is external).  Everything runs in the dtype of x and params, under autograd when they require it.
    masks:  {bn name: bool [B, cin, H, W]}: the ReLU after that BN is bn(x) * mask.
    drops:  {op name: [B, cout]} Dropout2d scales multiplied into that op's output.
    targets / target_idx / loss_scale: per BN group, for an op with a Gaussian-loss epilogue: targets[g]
    [rows, H, W], target_idx[g] the row of each sample of the group (None: identity), loss_scale[g]."""
    B = x.shape[0]
    groups = list(groups or [B])
    assert sum(groups) == B
    res = Result()
    bufs = {}
    for b in prog.buffers:
        bufs[id(b)] = torch.zeros(B, b.C, b.H, b.W, dtype=x.dtype)
    bufs[id(prog.input)] = x
    for op in prog.ops:
        src = bufs[id(op.src)][:, op.c0:op.c0 + op.cin]
        if op.bn is not None:
            z = _bn(src, groups, params[op.bn + '.weight'], params[op.bn + '.bias'])
            if masks is not None and op.bn in masks:
                m = masks[op.bn].to(torch.bool)
                assert m.shape == z.shape, (op.bn, tuple(m.shape), tuple(z.shape))
                zd = z.detach()
                dis = m != (zd > 0)
                res.audit.append((op.bn, int(dis.sum()), float(zd.abs()[dis].max()) if dis.any() else 0.0,
                                  z.numel()))
                src = z * m.to(z.dtype)
            else:
                src = torch.relu(z)
        if op.upsample:
            src = F.interpolate(src, scale_factor=2.0, mode='nearest')
        y = F.conv2d(src, params[op.w], stride=op.stride, padding=op.pad)
        if drops is not None and op.name in drops:
            y = y * drops[op.name].to(y.dtype)[:, :, None, None]
        # clone-and-assign: several ops may write disjoint channels of one buffer, and an op may read the
        # buffer it writes (src above is a view of the version before this op); autograd sees every version
        dst = bufs[id(op.dst)].clone()
        dst[:, op.d0:op.d0 + op.cout] = y
        bufs[id(op.dst)] = dst
        if op.epilogue in (EPI_GAUSS_LOSS, EPI_GAUSS_EXP_LOSS):
            assert op.cout == 2 and targets is not None
            logl = []
            s = 0
            for g, n in enumerate(groups):
                t = targets[g].to(y.dtype).reshape(-1, y.shape[2], y.shape[3])
                if target_idx is not None and target_idx[g] is not None:
                    t = t[torch.as_tensor(target_idx[g], dtype=torch.long)]
                logl.append(gauss_logl(y[s:s + n], t[:n], op.epilogue == EPI_GAUSS_EXP_LOSS))
                s += n
            res.logl = torch.stack(logl)
            scale = torch.ones(len(groups), dtype=y.dtype) if loss_scale is None else \
                torch.as_tensor(loss_scale, dtype=y.dtype)
            res.objective = -(scale * res.logl).sum()
    res.bufs = {b.name: bufs[id(b)] for b in prog.buffers}
    res.output = bufs[id(prog.output)]
    return res


def run_program(prog, params, x, groups=None, **kw):
    """The program's output buffer (evaluate's other results dropped)."""
    return evaluate(prog, params, x, groups, **kw).output
