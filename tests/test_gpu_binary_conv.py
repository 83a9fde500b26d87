"""Per-operator parity of the Bernoulli decoder likelihood (GPI_EPI_BERNOULLI_LOSS, include/gpi.h): the rows of
tests/conv_cases_binary.py through the machinery of tests/test_gpu_conv_ops.py -- separate launches
(gpi_codec_forward / gpi_codec_backward) and the fused output conv (gpi_conv_loss_fused, the kernel's one-channel
instantiation) against the same chain in fp64 (tests/program_interp.py with the loss op as a plain store, the
Bernoulli term in the logit form applied to its differentiable output, the kernels' ReLU decisions).

Bars, the project's per-operator ones: log-likelihood per group 1e-5, every parameter and input gradient 5e-5
per tensor, fused against separate launches 1e-6 (value) / 4e-6 (gradient tensors); a sentinel-filled workspace
in which nothing outside the ops' own buffers changes; cout = 2 with the Bernoulli epilogue is GPI_ERR_ARG.
Every logit stays below 15 in magnitude (asserted): above ~16.7 a fp32 sigmoid + clamped BCE, the reference's
form, deliberately differs from the logit form.  The first two tests are host-side (no GPU)."""
import ctypes as C

import pytest
import torch

from gpi import _lib as L
from gpi.engine import make_ctx
import conv_cases as cc
import conv_cases_binary as cb
from program_interp import evaluate

GPI_ERR_ARG = -1


def _plan(case, chain):
    lib = L.lib()
    fields = cc.shape_fields()
    prog = chain(case)
    ws, g, descs = cc.lay_out(case, prog)
    ctx = cc.plan_ctx(g)
    d = descs[prog.ops.index(prog.T)]
    out = {}
    for what, fwd, fuse in (('fwd', 1, 0), ('bwd', 0, 0), ('fuse', 0, 1)):
        if fuse:
            d.out_off = -1
        rc, s = cc.plan_shape(lib, d, ctx, fwd, fuse, fields)
        assert rc == 0, (case.id, what, rc)
        out[what] = s
    return out


@pytest.mark.parametrize('case', cb.CASES, ids=[c.id for c in cb.CASES])
def test_rows_plan_as_their_gaussian_twins(case):
    """Host side: each row plans, its fused launch is the Bernoulli form (exf == 2) of a one-channel op, and every
    launch takes the tile geometry (half tiles, rows per tile) of the Gaussian row it mirrors."""
    got, twin = _plan(case, cb.chain), _plan(cb.gauss_twin(case), cc.chain)
    assert got['fuse']['exf'] == 2 and got['fuse']['fusek'] == 1 and got['fuse']['D_cout'] == 1
    assert got['fuse']['D_epilogue'] == L.EPI_BERNOULLI_LOSS
    assert twin['fuse']['exf'] in (0, 1)
    for what in ('fwd', 'bwd', 'fuse'):
        for k in ('half', 'G_th', 'G_tiles', 'G_npx'):
            assert got[what][k] == twin[what][k], (case.id, what, k, got[what][k], twin[what][k])
    table = set(cc.parse_shapes(open(cc.CONV_SHAPES_H).read()))
    assert all(s['_row'] not in table for s in got.values()), 'the rows run the generic kernels'


def test_bernoulli_epilogue_argument_checks():
    """cout != 1 or a BN-backward output gradient with the Bernoulli epilogue: GPI_ERR_ARG, in every launch form."""
    lib = L.lib()
    case = cb.CASES[0]
    prog = cb.chain(case)
    ws, g, descs = cc.lay_out(case, prog)
    ctx = cc.plan_ctx(g)
    d = L.ConvDesc.from_buffer_copy(descs[prog.ops.index(prog.T)])
    d.cout = 2
    for fwd, fuse in ((1, 0), (0, 0), (0, 1)):
        assert lib.gpi_conv_shape_plan(C.byref(d), C.byref(ctx), fwd, fuse) == GPI_ERR_ARG
    d.cout, d.gout_mode = 1, 0
    assert lib.gpi_conv_shape_plan(C.byref(d), C.byref(ctx), 1, 0) == GPI_ERR_ARG


def _patch(monkeypatch, ops, case):
    """test_gpu_conv_ops's run / check functions on the Bernoulli rows: this table's chain, two-valued targets,
    tgt_lo in the context, and the Bernoulli term as the reference's loss."""
    real_inputs, real_ctx = ops._inputs, make_ctx

    def inputs(c, prog):
        d = real_inputs(c, prog)
        d['targets'] = cb.two_valued_targets(c, d['targets'], c.seed)
        return d

    def ctx_with_lo(ws, flat, groups):
        ctx = real_ctx(ws, flat, groups)
        for gi in range(len(groups)):
            ctx.tgt_lo[gi] = case.lo[gi]
        return ctx

    def reference(c, r, masks, dtype=torch.float64):
        inp, prog = r['inp'], r['prog']
        p = {n: v.to(dtype).requires_grad_(True) for n, v in inp['params'].items()}
        x = inp['x'].to(dtype).requires_grad_(True)
        res = evaluate(prog, p, x, c.groups, masks=masks, drops=inp['drops'])
        assert res.logl is None, 'the interpreter stores the Bernoulli op plainly'
        a = res.output
        assert float(a.detach().abs().max()) < cb.LOGIT_MAX
        tg = [t.to(dtype) for t in inp['targets']]
        res.logl, res.objective = cb.bernoulli_terms(a, tg, inp['tgt_idx'], c.groups, c.lo, inp['loss_scale'])
        res.objective.backward()
        grads = {n: v.grad.detach().numpy() for n, v in p.items()}
        grads['input'] = x.grad.detach().numpy()
        return res, grads

    monkeypatch.setattr(ops, 'chain', cb.chain)
    monkeypatch.setattr(ops, '_inputs', inputs)
    monkeypatch.setattr(ops, 'make_ctx', ctx_with_lo)
    monkeypatch.setattr(ops, 'reference', reference)


@pytest.mark.gpu
@pytest.mark.parametrize('case', cb.CASES, ids=[c.id for c in cb.CASES])
def test_bernoulli_conv_case(case, device, monkeypatch):
    import test_gpu_conv_ops as ops
    from elbo_ref import tensor_rel
    _patch(monkeypatch, ops, case)
    sep = ops.check_run(case, ops.run_gpu(case, device))
    fus = ops.check_run(case, ops.run_gpu(case, device, fused=True))
    for gi in range(len(case.groups)):
        assert abs(fus[2][gi] - sep[2][gi]) <= 1e-6 * abs(sep[2][gi]), (case.id, gi, fus[2][gi], sep[2][gi])
    worst = 0.0
    for name, t in sep[1].items():
        err = tensor_rel(fus[1][name], t)
        worst = max(worst, err)
        assert err <= 4e-6, (case.id, name, err)
    print('%s fused vs separate: worst gradient tensor %.2e' % (case.id, worst))


@pytest.mark.gpu
def test_two_channel_bernoulli_op_is_refused_on_the_device(device):
    """The launch entry points themselves (not only the planner) return GPI_ERR_ARG for cout = 2 and launch
    nothing: a sentinel-filled workspace stays as it is."""
    import test_gpu_conv_ops as ops
    from gpi.flat import FlatParameters
    lib = L.lib()
    case = cb.CASES[1]
    prog = cb.chain(case)
    named = [(n, torch.nn.Parameter(torch.zeros(s))) for n, s in cc.param_shapes(prog)]
    flat = FlatParameters(named, device)
    ws, g, descs = cc.lay_out(case, prog, lambda name: flat.name_offsets[name])
    ws.materialize(device)
    ws.t_ws.fill_(ops.SENT)
    ctx = make_ctx(ws, flat, case.groups)
    tgt = torch.zeros(case.B, case.h, case.w, device=device)
    ctx.tgt[0] = tgt.data_ptr()
    d = L.ConvDesc.from_buffer_copy(descs[prog.ops.index(prog.T)])
    d.cout = 2
    st = L.stream_handle()
    assert lib.gpi_conv_forward(C.byref(d), C.byref(ctx), st) == GPI_ERR_ARG
    assert lib.gpi_conv_loss_fused(C.byref(d), C.byref(ctx), st) == GPI_ERR_ARG
    torch.cuda.synchronize()
    assert bool((ws.t_ws == ops.SENT).all())
