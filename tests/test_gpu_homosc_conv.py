"""Per-operator parity of the homoscedastic decoder likelihood (GPI_EPI_GAUSS_HOMO_LOSS / GPI_EPI_GAUSS_HOMO_EXP_LOSS,
include/gpi.h): the rows of tests/conv_cases_homosc.py through the machinery of tests/test_gpu_conv_ops.py --
separate launches (gpi_codec_forward / gpi_codec_backward / gpi_wgrad_reduce) and the fused output conv
(gpi_conv_loss_fused, the kernel's one-channel instantiations EXF 3 / 4) against the same chain in fp64
(tests/program_interp.py with the loss op as a plain store, the homoscedastic Gaussian term applied to its
differentiable output and the plane parameter, the kernels' ReLU decisions).

Bars, the project's per-operator ones: stored buffers 1e-5, log-likelihood per group 1e-5, every parameter (the plane
included) and input gradient 5e-5 per tensor, fused against separate launches 1e-6 (value) / 4e-6 (gradient
tensors).  The per-sample d/d(log sigma) rows in the slab buffer -- not only their sum -- against fp64 at 5e-5 of
the rows' maximum (a wrong row or tile offset moves whole rows).  Sentinel-filled workspace and slab buffer:
nothing outside the ops' own buffers, slab rows and the per-sample rows changes, and every (sample, pixel) of the
rows is written; with gls_off = -1 the rows' region stays untouched too.  Two runs are bit-identical."""
import numpy as np
import pytest
import torch

from gpi.engine import make_ctx
import conv_cases as cc
import conv_cases_homosc as ch
from program_interp import evaluate

pytestmark = pytest.mark.gpu


def _patch(monkeypatch, ops, case, rows=True):
    """test_gpu_conv_ops's run / check functions on the homoscedastic rows: this table's chain and parameters (the
    plane ~ N(-1, 0.3)), the per-sample rows allocated behind the slabs and reduced with them, ls_off / gls_off in
    the context, and the homoscedastic term as the reference's loss.  rows False: gls_off = -1 (the region is
    still allocated, nothing may write it, nothing reduces it)."""
    real_inputs, real_ctx, real_lay_out = ops._inputs, make_ctx, cc.lay_out
    state = {}

    def inputs(c, prog):
        d = real_inputs(c, prog)
        gen = torch.Generator().manual_seed(3000 + c.seed)
        d['params'][ch.PLANE] = (-1.0 + 0.3 * torch.randn(c.h, c.w, generator=gen)).float()
        return d

    def lay_out(c, prog, param_offset=None):
        ws, g, descs = real_lay_out(c, prog, param_offset)
        prog.gls_off = ws.parts.alloc(c.B * c.h * c.w)
        state['prog'] = prog
        if rows:
            plain = prog.reduce_items
            prog.reduce_items = lambda off: plain(off) + [ch.plane_reduce_item(prog, c.B, off)]
        return ws, g, descs

    def ctx_with_plane(ws, flat, groups):
        ctx = real_ctx(ws, flat, groups)
        ctx.ls_off = flat.name_offsets[ch.PLANE]
        ctx.gls_off = state['prog'].gls_off if rows else -1
        return ctx

    def reference(c, r, masks, dtype=torch.float64):
        inp, prog = r['inp'], r['prog']
        p = {n: v.to(dtype).requires_grad_(True) for n, v in inp['params'].items()}
        x = inp['x'].to(dtype).requires_grad_(True)
        res = evaluate(prog, p, x, c.groups, masks=masks, drops=inp['drops'])
        assert res.logl is None, 'the interpreter stores the homoscedastic op plainly'
        res.logl, res.objective, res.gls_rows = ch.homosc_terms(res.output, p[ch.PLANE], inp['targets'], inp['tgt_idx'],
                                                                c.groups, c.exp_field, inp['loss_scale'])
        res.objective.backward()
        grads = {n: v.grad.detach().numpy() for n, v in p.items()}
        grads['input'] = x.grad.detach().numpy()
        state['rows_ref'] = res.gls_rows.numpy()
        return res, grads

    monkeypatch.setattr(ops, 'chain', ch.chain)
    monkeypatch.setattr(ops, 'param_shapes', ch.param_shapes)
    monkeypatch.setattr(ops, 'lay_out', lay_out)
    monkeypatch.setattr(ops, '_inputs', inputs)
    monkeypatch.setattr(ops, 'make_ctx', ctx_with_plane)
    monkeypatch.setattr(ops, 'reference', reference)
    return state


def _parts(r):
    return r['ws'].t_parts.cpu().numpy()


def _rows_region(case, r):
    o = r['prog'].gls_off
    return _parts(r)[o:o + case.B * case.h * case.w].reshape(case.B, case.h * case.w)


def _check_parts(ops, case, r, rows):
    """The slab buffer: everything outside the ops' slab rows and the per-sample rows still holds the sentinel;
    the per-sample rows are all written (rows) or all untouched (gls_off = -1)."""
    parts = _parts(r)
    own = np.zeros(parts.size, bool)
    for op in r['prog'].ops:
        own[op.desc.wpart_off:op.desc.wpart_off + op.blocks * op.rowlen] = True
    o, n = r['prog'].gls_off, case.B * case.h * case.w
    assert not own[o:o + n].any(), 'the per-sample rows overlap a slab'
    region = parts[o:o + n]
    if rows:
        assert (region != np.float32(ops.SENT)).all(), '%s: %d of the per-sample row elements never written' % (
            case.id, int((region == np.float32(ops.SENT)).sum()))
        own[o:o + n] = True
    stray = np.flatnonzero(~own & (parts != np.float32(ops.SENT)))
    assert stray.size == 0, '%s: %d slab-buffer elements nobody owns were written, first at %d (rows at %d)' % (
        case.id, stray.size, stray[0], o)


@pytest.mark.parametrize('case', ch.CASES, ids=[c.id for c in ch.CASES])
def test_homosc_conv_case(case, device, monkeypatch):
    import test_gpu_conv_ops as ops
    from elbo_ref import tensor_rel
    state = _patch(monkeypatch, ops, case)
    runs = {}
    for fused in (False, True):
        r = ops.run_gpu(case, device, fused=fused)
        out = ops.check_run(case, r)
        err = tensor_rel(_rows_region(case, r), state['rows_ref'])
        print('%s%s per-sample d/dlogsigma rows vs fp64: %.2e' % (case.id, ' (fused)' if fused else '', err))
        assert err <= 5e-5, (case.id, fused, err)
        _check_parts(ops, case, r, True)
        runs[fused] = (r, out)
    sep, fus = runs[False][1], runs[True][1]
    for gi in range(len(case.groups)):
        assert abs(fus[2][gi] - sep[2][gi]) <= 1e-6 * abs(sep[2][gi]), (case.id, gi, fus[2][gi], sep[2][gi])
    worst = 0.0
    for name, t in sep[1].items():
        err = tensor_rel(fus[1][name], t)
        worst = max(worst, err)
        assert err <= 4e-6, (case.id, name, err)
    print('%s fused vs separate: worst gradient tensor %.2e' % (case.id, worst))
    # a second fused run: bit-identical values, gradients (the plane's included) and per-sample rows
    r2 = ops.run_gpu(case, device, fused=True)
    r1 = runs[True][0]
    assert r1['logl'].tobytes() == r2['logl'].tobytes()
    assert r1['gacc'].tobytes() == r2['gacc'].tobytes()
    assert _rows_region(case, r1).tobytes() == _rows_region(case, r2).tobytes()


@pytest.mark.parametrize('fused', [False, True], ids=['separate', 'fused'])
@pytest.mark.parametrize('case', [ch.CASES[0], ch.CASES[7]], ids=[ch.CASES[0].id, ch.CASES[7].id])
def test_without_gls_rows_nothing_is_written_beyond_the_slabs(case, fused, device, monkeypatch):
    """gls_off = -1 (the input-gradient-only engines): the per-sample rows' region keeps the sentinel, the plane's
    gradient stays zero, and every other result equals the run with rows bit for bit."""
    import test_gpu_conv_ops as ops
    _patch(monkeypatch, ops, case, rows=True)
    with_rows = ops.run_gpu(case, device, fused=fused)
    monkeypatch.undo()
    _patch(monkeypatch, ops, case, rows=False)
    r = ops.run_gpu(case, device, fused=fused)
    _check_parts(ops, case, r, False)
    assert (_rows_region(case, r) == np.float32(ops.SENT)).all()
    o = r['offset'](ch.PLANE)
    n = case.h * case.w
    assert not r['gacc'][o:o + n].any()
    assert np.abs(with_rows['gacc'][o:o + n]).max() > 0
    assert r['logl'].tobytes() == with_rows['logl'].tobytes()
    keep = np.ones(r['gacc'].size, bool)
    keep[o:o + n] = False
    assert r['gacc'][keep].tobytes() == with_rows['gacc'][keep].tobytes()
    assert r['ws_np'].tobytes() == with_rows['ws_np'].tobytes()
