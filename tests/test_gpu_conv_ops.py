"""Per-operator conv parity sweep: every case of tests/conv_cases.py (one conv under test inside a tiny
producer / consumer chain, each chosen to reach a kernel-variant combination of conv.hip the shipped
configurations never run) on the GPU -- gpi_codec_forward, gpi_codec_backward, gpi_wgrad_reduce on the
laid-out program, as DecoderEngine runs its own minus the head -- against a plain fp64 evaluation of the
same program (tests/program_interp.py) with the kernels' ReLU decisions (tests/gpu_masks.py).

Bars (the project's stated parity bars, per-tensor max-norm relative error, elbo_ref.tensor_rel):
  forward   every stored buffer, the channels each op wrote                      1e-5
            BN batch sums (sum, sumsq) against fp64 sums of the stored values     1e-6
            Gaussian log-likelihood per group (loss rows)                         1e-5
  backward  every parameter gradient (producers and consumer included) and the
            internal input's gradient buffer                                      5e-5
            fused output conv against the separate launches            1e-6 value, 4e-6 per tensor
ReLU decisions: adopted from the kernels, and allowed to differ from the fp64 run's own only where
|bn(x)| < 1e-4, in at most max(2, 1e-4 n) elements per layer (a condition, not a tolerance).
Untouched memory: the workspace is filled with a sentinel before the forward; everything no op owns
(channels no op writes, the alignment gaps between buffers) must still hold it afterwards, and everything an
op owns must not.  tests/test_conv_cases_plan.py proves on the host which variant each case reaches."""
import ctypes as C

import numpy as np
import pytest
import torch

from gpi import _lib as L
from gpi.engine import N_TERMS, make_ctx, run_reduce
from gpi.flat import FlatParameters
from conv_cases import CASES, REFUSALS, DROP_P, chain, lay_out, param_shapes
from elbo_ref import tensor_rel
from gpu_masks import _program_masks, replica_sums
from program_interp import evaluate

pytestmark = pytest.mark.gpu

SENT = -7777.0
BARS = {'fwd': 1e-5, 'stat': 1e-6, 'logl': 1e-5, 'grad': 5e-5}
AUDIT_ABS = 1e-4
GPI_ERR_UNSUPPORTED = -3


def _inputs(case, prog):
    """CPU fp32 tensors of a case, all from the case's seed: parameters, input (internal z, or the external
    image pool and its row index), Dropout2d scales, upstream gradient or loss targets."""
    gen = torch.Generator().manual_seed(1000 + case.seed)
    rng = np.random.RandomState(case.seed)
    B = case.B
    d = {'params': {}}
    for name, shape in param_shapes(prog):
        if len(shape) == 4:
            v = torch.randn(shape, generator=gen) / float(np.sqrt(shape[1] * shape[2] * shape[3]))
        elif name.endswith('.weight'):
            v = (0.5 + torch.rand(shape, generator=gen)) * (torch.randint(0, 2, shape, generator=gen) * 2 - 1).float()
        else:
            v = torch.randn(shape, generator=gen) * float(np.sqrt(0.5))
        d['params'][name] = v.float()
    if case.ext:
        rows = B + 3 if case.shuffle else B
        d['pool'] = torch.randn(rows, case.h * case.w, generator=gen)
        d['ext_idx'] = torch.tensor(rng.permutation(rows)[:B].astype(np.int32)) if case.shuffle else None
        idx = d['ext_idx'].long() if case.shuffle else torch.arange(B)
        d['x'] = d['pool'][idx].reshape(B, 1, case.h, case.w)
    else:
        d['x'] = torch.randn(B, 4, case.h, case.w, generator=gen)
    d['drops'] = {}
    for op in prog.ops:
        if op.drop:
            keep = rng.rand(B, op.cout) >= DROP_P
            keep[B // 2] = False                 # one sample with every channel dropped
            keep[0, 0], keep[0, -1] = True, False
            d['drops'][op.name] = torch.tensor(keep.astype(np.float32) / np.float32(1.0 - DROP_P))
    o = prog.output
    if case.loss:
        d['targets'], d['tgt_idx'] = [], []
        for g, n in enumerate(case.groups):
            shuf = case.shuffle and g == 0
            rows = n + 3 if shuf else n
            d['targets'].append(torch.randn(rows, o.H, o.W, generator=gen))
            d['tgt_idx'].append(torch.tensor(rng.permutation(rows)[:n].astype(np.int32)) if shuf else None)
        d['loss_scale'] = list(case.loss_scale or [1.0] * len(case.groups))
    else:
        d['R'] = torch.randn(B, o.C, o.H, o.W, generator=gen)
    return d


def _owned(case, prog, size, fused):
    """Boolean map of the workspace elements some op (or the test's own setup) writes."""
    B = case.B
    own = np.zeros(size, bool)

    def mark(off, b, c0, n):
        v = own[off:off + B * b.per_sample].reshape(B, b.C, b.H * b.W)
        v[:, c0:c0 + n] = True

    if not prog.input.external:
        mark(prog.input.off, prog.input, 0, prog.input.C)
    for op in prog.ops:
        if not (fused and op is prog.T):
            mark(op.dst.off, op.dst, op.d0, op.cout)
        if op.desc.gin_off >= 0:
            mark(op.src.s_off, op.src, op.c0, op.cin)
        if op.drop:
            own[op.drop_off:op.drop_off + B * op.cout] = True
    if prog.output.s_off is not None and not fused:     # (fused: the output gradient never leaves LDS)
        mark(prog.output.s_off, prog.output, 0, prog.output.C)
    return own


def run_gpu(case, device, fused=False):
    """One forward (+ backward + slab reduction) of the case's program on the GPU; the raw results."""
    lib = L.lib()
    prog = chain(case)
    inp = _inputs(case, prog)
    named = [(n, torch.nn.Parameter(v.clone())) for n, v in inp['params'].items()]
    flat = FlatParameters(named, device)
    offset = lambda name: flat.name_offsets[name]
    ws, g, descs = lay_out(case, prog, offset)
    ws.materialize(device)
    ws.t_ws.fill_(SENT)
    ws.t_parts.fill_(SENT)
    ctx = make_ctx(ws, flat, case.groups)
    B, n_ops = case.B, len(descs)
    hold = []

    def dev(t):
        t = t.contiguous().to(device)
        hold.append(t)
        return t

    if case.ext:
        ctx.ext_in = dev(inp['pool']).data_ptr()
        ctx.ext_stride = case.h * case.w
        if inp['ext_idx'] is not None:
            ctx.ext_idx = dev(inp['ext_idx']).data_ptr()
    else:
        z = prog.input
        ws.view(z.off, B, z.C, z.H, z.W).copy_(inp['x'])
    for op in prog.ops:
        if op.drop:
            ws.view(op.drop_off, B, op.cout).copy_(inp['drops'][op.name])
    o = prog.output
    if case.loss:
        for gi in range(len(case.groups)):
            ctx.tgt[gi] = dev(inp['targets'][gi]).data_ptr()
            if inp['tgt_idx'][gi] is not None:
                ctx.tgt_idx[gi] = dev(inp['tgt_idx'][gi]).data_ptr()
            ctx.loss_scale[gi] = inp['loss_scale'][gi]
    elif case.grad:
        ws.view(o.s_off, B, o.C, o.H, o.W).copy_(inp['R'])
    st = L.stream_handle()
    ws.zero_scratch()
    flat.gacc.zero_()
    n_plain = n_ops - 1 if fused else n_ops
    L.check(lib.gpi_codec_forward(descs, n_plain, C.byref(ctx), st), 'forward ' + case.id)
    if fused:
        descs[n_ops - 1].out_off = -1        # as the engine: the fused loss epilogue writes no output image
        L.check(lib.gpi_conv_loss_fused(C.byref(descs[n_ops - 1]), C.byref(ctx), st), 'fused ' + case.id)
    if case.grad:
        L.check(lib.gpi_codec_backward(descs, n_plain, C.byref(ctx), st), 'backward ' + case.id)
        run_reduce(prog.reduce_items(offset), ws, flat, st)
    torch.cuda.synchronize()
    scr = ws.t_scr.cpu().numpy()
    R_, G_ = L.GPI_REPLICAS, L.GPI_MAX_GROUPS
    s0 = N_TERMS * R_
    return dict(prog=prog, inp=inp, flat=flat, ws=ws, ws_np=ws.t_ws.cpu().numpy(), fused=fused,
                stats=replica_sums(scr[s0:s0 + R_ * G_ * ws.n_stats * 4].reshape(R_, G_, ws.n_stats, 4)),
                logl=scr[:s0].reshape(N_TERMS, R_).sum(1)[:len(case.groups)],
                gacc=flat.gacc.cpu().numpy(), P=flat.P.detach().cpu().numpy(), offset=offset)


def kernel_masks(case, r):
    """The kernels' ReLU decisions of every BN layer, [B, cin, H, W] over all groups."""
    per_group = []
    s = 0
    for gi, n in enumerate(case.groups):
        per_group.append(_program_masks(r['prog'], r['ws_np'], r['stats'], r['P'], slice(s, s + n), gi, n))
        s += n
    return {k: torch.cat([m[k] for m in per_group], 0) for k in per_group[0]}


def reference(case, r, masks, dtype=torch.float64):
    """The same program in plain torch on the CPU (dtype fp64: the reference; fp32: how far plain fp32
    arithmetic is from it), with the given ReLU decisions; gradients of the objective when the case has a
    backward."""
    inp, prog = r['inp'], r['prog']
    p = {n: v.to(dtype).requires_grad_(case.grad) for n, v in inp['params'].items()}
    x = inp['x'].to(dtype).requires_grad_(case.grad and not case.ext)
    kw = {}
    if case.loss:
        kw = dict(targets=inp['targets'], target_idx=inp['tgt_idx'], loss_scale=inp['loss_scale'])
    res = evaluate(prog, p, x, case.groups, masks=masks, drops=inp['drops'], **kw)
    grads = {}
    if case.grad:
        obj = res.objective if case.loss else (res.output * inp['R'].to(dtype)).sum()
        obj.backward()
        grads = {n: v.grad.detach().numpy() for n, v in p.items()}
        if not case.ext:
            grads['input'] = x.grad.detach().numpy()
    return res, grads


def gpu_tensors(case, r):
    """(forward tensors, gradient tensors) of a GPU run, keyed as errors() keys the reference's."""
    prog, ws_np, B = r['prog'], r['ws_np'], case.B
    view = lambda off, b: ws_np[off:off + B * b.per_sample].reshape(B, b.C, b.H, b.W)
    fwd = {}
    for op in prog.ops:
        if not (r['fused'] and op is prog.T):
            fwd[op.name] = view(op.dst.off, op.dst)[:, op.d0:op.d0 + op.cout]
    grads = {}
    if case.grad:
        for name, shape in param_shapes(prog):
            o = r['offset'](name)
            grads[name] = r['gacc'][o:o + int(np.prod(shape))].reshape(shape)
        if not case.ext:
            grads['input'] = view(prog.input.s_off, prog.input)
    return fwd, grads


def errors(case, fwd, grads, logl, res, ref_grads):
    """{check: (error, bar class)} of forward tensors, log-likelihoods and gradients against a reference run."""
    e = {}
    for name, t in fwd.items():
        e['fwd ' + name] = (tensor_rel(t, _ref_fwd(res, name)), 'fwd')
    if case.loss:
        ref = res.logl.detach().numpy()
        for gi in range(len(case.groups)):
            e['logl group %d' % gi] = (abs(logl[gi] - ref[gi]) / abs(ref[gi]), 'logl')
    for name, t in grads.items():
        e['grad ' + name] = (tensor_rel(t, ref_grads[name]), 'grad')
    return e


def _ref_fwd(res, name):
    op = res.ops[name]
    return res.bufs[op.dst.name].detach().numpy()[:, op.d0:op.d0 + op.cout]


def stat_errors(case, r):
    """BN batch sums of every statistics record against fp64 sums of the stored fp32 activations; the records
    of channels no op writes must be untouched (zero)."""
    prog, B = r['prog'], case.B
    e = {}
    for b in prog.buffers:
        if b.stat is None:
            continue
        written = np.zeros(b.C, bool)
        for op in prog.ops:
            if op.dst is b and not (r['fused'] and op is prog.T):
                written[op.d0:op.d0 + op.cout] = True
        a = r['ws_np'][b.off:b.off + B * b.per_sample].reshape(B, b.C, -1).astype(np.float64)
        ref = np.zeros((len(case.groups), b.C, 2))
        s = 0
        for gi, n in enumerate(case.groups):
            ref[gi, :, 0] = a[s:s + n].sum((0, 2))
            ref[gi, :, 1] = (a[s:s + n] ** 2).sum((0, 2))
            s += n
        got = r['stats'][:len(case.groups), b.stat:b.stat + b.C, :2]
        assert not got[:, ~written].any(), 'statistics of unwritten channels of %s touched' % b.name
        for k, what in enumerate(('sum', 'sumsq')):
            e['stat %s %s' % (b.name, what)] = (tensor_rel(got[:, written, k], ref[:, written, k]), 'stat')
    return e


def check_untouched(case, r):
    own = _owned(case, r['prog'], r['ws_np'].size, r['fused'])
    ws_np = r['ws_np']
    stray = np.flatnonzero(~own & (ws_np != np.float32(SENT)))
    assert stray.size == 0, '%s: %d workspace elements no op owns were written, first at %d (allocations %r)' % (
        case.id, stray.size, stray[0], r['ws'].ws.allocs)
    missed = np.flatnonzero(own & (ws_np == np.float32(SENT)))
    assert missed.size == 0, '%s: %d owned workspace elements never written, first at %d (allocations %r)' % (
        case.id, missed.size, missed[0], r['ws'].ws.allocs)


def check_run(case, r):
    """All checks of one GPU run against the fp64 reference; returns (gpu forward, gpu gradients, logl)."""
    prog = r['prog']
    masks = kernel_masks(case, r)
    res, ref_grads = reference(case, r, masks)
    res.ops = {op.name: op for op in prog.ops}
    for name, n_dis, worst, n in res.audit:
        print('%s mask audit %s: %d of %d decisions differ, largest |bn(x)| %.2e' % (case.id, name, n_dis, n, worst))
        assert worst < AUDIT_ABS and n_dis <= max(2, 1e-4 * n), (case.id, name, n_dis, worst, n)
    fwd, grads = gpu_tensors(case, r)
    e = errors(case, fwd, grads, r['logl'], res, ref_grads)
    e.update(stat_errors(case, r))
    worst = {c: max([v for v, cls in e.values() if cls == c] or [0.0]) for c in BARS}
    print('%s%s worst errors: forward %.2e, statistics %.2e%s%s' % (
        case.id, ' (fused)' if r['fused'] else '', worst['fwd'], worst['stat'],
        ', logL %.2e' % worst['logl'] if case.loss else '', ', gradient %.2e' % worst['grad'] if case.grad else ''))
    bars = dict(BARS, **case.bars)
    bad = {k: v for k, (v, cls) in e.items() if not v <= bars[cls]}
    if bad:
        # rounding or a bug?  the same chain in plain fp32 torch on the CPU, same decisions, against fp64
        res32, g32 = reference(case, r, masks, torch.float32)
        res32.ops = res.ops
        f32 = {n: _ref_fwd(res32, n) for n in fwd}
        l32 = res32.logl.detach().numpy() if case.loss else None
        e32 = errors(case, f32, g32, l32, res, ref_grads)
        pytest.fail('%s%s over its bar: %s' % (case.id, ' (fused)' if r['fused'] else '', '; '.join(
            '%s %.3e (bar %.0e, plain fp32 torch %.3e)' % (k, v, bars[e[k][1]], e32.get(k, (float('nan'),))[0])
            for k, v in bad.items())))
    check_untouched(case, r)
    return fwd, grads, r['logl']


@pytest.mark.parametrize('case', CASES, ids=[c.id for c in CASES])
def test_conv_case(case, device):
    for cls, bar in case.bars.items():
        assert bar <= 10 * BARS[cls], 'a raised bar is capped at 10x the project bar'
    sep = check_run(case, run_gpu(case, device))
    if case.loss:
        # gpi_conv_loss_fused in place of T's two launches: against fp64 as above, and against the separate
        # launches at the bars of test_fused_output_conv_matches_separate_launches
        fus = check_run(case, run_gpu(case, device, fused=True))
        for gi in range(len(case.groups)):
            assert abs(fus[2][gi] - sep[2][gi]) <= 1e-6 * abs(sep[2][gi]), (case.id, gi, fus[2][gi], sep[2][gi])
        worst = 0.0
        for name, t in sep[1].items():
            err = tensor_rel(fus[1][name], t)
            worst = max(worst, err)
            assert err <= 4e-6, (case.id, name, err)
        print('%s fused vs separate: worst gradient tensor %.2e' % (case.id, worst))


@pytest.mark.parametrize('case', REFUSALS, ids=[c.id for c in REFUSALS])
def test_refused_backward_leaves_memory_alone(case, device):
    lib = L.lib()
    prog = chain(case)
    named = [(n, torch.nn.Parameter(torch.zeros(s))) for n, s in param_shapes(prog)]
    flat = FlatParameters(named, device)
    ws, g, descs = lay_out(case, prog, lambda name: flat.name_offsets[name])
    ws.materialize(device)
    ws.t_ws.fill_(SENT)
    ws.t_parts.fill_(SENT)
    flat.gacc.fill_(SENT)
    ctx = make_ctx(ws, flat, case.groups)
    d = descs[prog.ops.index(prog.T)]
    assert lib.gpi_conv_backward(C.byref(d), C.byref(ctx), L.stream_handle()) == GPI_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    for t in (flat.gacc, ws.t_parts, ws.t_ws):
        assert bool((t == SENT).all())
