"""Operator-level sweep of the dense head: gpi_head_forward, gpi_head_backward and gpi_outer_gemm in every kernel
form against the fp64 reference (tests/head_ref.py) over the case table of tests/head_cases.py -- 8 layouts x 26
(counts, mode) cases, and 81 bare gpi_outer_gemm launches.

Per case and form (default dispatch: the form the table names, asserted through gpi_head_form; GPI_HEAD_VALU plus
item-0 flag 2: the per-sample VALU kernels and the scalar GEMM tiles):
  * every output region, each of the seven term sums and every gradient tensor against the reference, the project's
    max|d| / max|ref|: 1e-5 outputs and terms, 5e-5 gradients; a reference that is identically zero is met exactly;
  * after each launch, every workspace float the mode does not write (by then) -- guard bands, inputs, rows of a
    segment without the term -- bit-equal to its initial state; the accumulator exactly 0 outside the parameter
    blocks and wherever the mode has no gradient;
  * the backward as GPI_HEAD_PART_ENC then GPI_HEAD_PART_Q launches on a fresh accumulator: the accumulator within
    1e-12 of the single launch's (per-row values are the same fp32 numbers: the fp64 sums differ at most by the
    order of the atomics), gfeat / dhpre / dzmu / dzls / gmux bit-equal.
Two child processes (the switches are read once per process) run the two family layouts through the generic MFMA
form (GPI_HEAD_PREFETCH=0) with the same comparisons, and check that with GPI_HEAD_MFMA=0 default dispatch equals
the GPI_HEAD_VALU run bit for bit.

Each test prints its measured maxima per region class (profiles/head_ops_parity.txt)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, PKG
import head_cases as H
import head_ref as R

pytestmark = pytest.mark.gpu
TESTS = os.path.dirname(os.path.abspath(__file__))
PART_REGIONS = ('gfeat', 'dhpre', 'dzmu', 'dzls', 'gmux')


class Runner:
    """One case's device buffers and launches."""

    def __init__(self, case, dev):
        from gpi import _lib as L
        self.L, self.lib, self.c, self.dev = L, L.lib(), case, dev
        self.st = L.stream_handle()
        self.P0, self.ws0 = case.param_vector(), case.workspace()
        self.P = torch.from_numpy(self.P0).to(dev)
        self.ws_init = torch.from_numpy(self.ws0).to(dev)
        self.ws = torch.empty_like(self.ws_init)
        self.gacc = torch.zeros(case.n_params, dtype=torch.float64, device=dev)
        self.terms = torch.zeros(7 * H.REPLICAS + H.NG, dtype=torch.float64, device=dev)

    def untouched(self, keep, what):
        """After a launch: every workspace float under the mask `keep` is bit-equal to its initial state."""
        torch.cuda.synchronize()
        same = self.ws.cpu().numpy().view(np.uint32) == self.ws0.view(np.uint32)
        assert same[keep].all(), (self.c.id, what, 'workspace floats outside the written rows changed',
                                  np.flatnonzero(~same & keep)[:8], {k: r.off for k, r in self.c.w_reg.items()})

    def run(self, valu, split=False, keep=None):
        """forward, backward (split: its two half-launches), outer GEMM -> (ws, terms, gacc) as numpy arrays.
        keep: masks (after the forward, after the backward / GEMM) of the floats a launch must leave alone."""
        L, lib, c = self.L, self.lib, self.c
        self.ws.copy_(self.ws_init)
        self.gacc.zero_()
        self.terms.zero_()
        extra = L.HEAD_VALU if valu else 0
        p = lambda t: L.ptr(t)
        hd = c.desc(L, self.terms.data_ptr(), extra)
        L.check(lib.gpi_head_forward(C.byref(hd), p(self.P), p(self.ws), self.st), 'head forward')
        if keep:
            self.untouched(keep[0], 'forward')
        for part in ((L.HEAD_PART_ENC, L.HEAD_PART_Q) if split else (0,)):
            hb = c.desc(L, self.terms.data_ptr(), extra | part)
            L.check(lib.gpi_head_backward(C.byref(hb), p(self.P), p(self.ws), p(self.gacc), self.st), 'head backward')
            if keep:
                self.untouched(keep[1], 'backward')
        items = c.gemm_items(L, valu)
        if len(items):
            L.check(lib.gpi_outer_gemm(items, len(items), p(self.ws), p(self.gacc), self.st), 'outer gemm')
        if keep:
            self.untouched(keep[1], 'outer gemm')
        torch.cuda.synchronize()
        assert (self.P.cpu().numpy().view(np.uint32) == self.P0.view(np.uint32)).all(), 'parameters written'
        return self.ws.cpu().numpy(), self.terms.cpu().numpy(), self.gacc.cpu().numpy()


def check_case(c, rn, valu):
    """All comparisons of one case in one form; returns the errors by key."""
    ref = c.reference()
    # what the mode does not write -- guard bands, inputs, rows without the term -- is untouched after each launch
    fwd, written = np.zeros(c.n_ws, dtype=bool), np.zeros(c.n_ws, dtype=bool)
    for k in R.FWD_REGIONS + R.BWD_REGIONS:
        c.w_reg[k].view(written)[...] = ~np.isnan(ref[k])
        if k in R.FWD_REGIONS:
            c.w_reg[k].view(fwd)[...] = ~np.isnan(ref[k])
    keep = (~fwd, ~written)
    ws, terms, gacc = rn.run(valu, keep=keep)
    got = c.extract(ws, terms, gacc)
    errs = H.compare(got, ref)
    bad = H.over_bar(errs)
    assert not bad, (c.id, 'valu' if valu else 'default', bad)
    assert not np.isnan(ws[written]).any(), c.id
    assert (gacc[~c.param_mask()] == 0).all(), (c.id, valu, 'accumulator written outside the parameter blocks')
    assert (terms[7 * H.REPLICAS:] == 0).all()
    # the two half-launches of the backward
    ws2, terms2, gacc2 = rn.run(valu, split=True, keep=keep)
    for k, r in c.p_reg.items():
        a, b = r.view(gacc2), r.view(gacc)
        den = np.abs(b).max() if b.size else 0.0
        assert (np.abs(a - b).max() if b.size else 0.0) <= 1e-12 * den, (c.id, valu, 'split backward', k)
    assert (gacc2[~c.param_mask()] == 0).all()
    for k in PART_REGIONS:
        assert (c.w_reg[k].view(ws2).view(np.uint32) == c.w_reg[k].view(ws).view(np.uint32)).all(), (c.id, valu, k)
    assert (terms2 == terms).all()
    return errs


def sweep(layout, valu, dev, expect_form=None, prefetch=1):
    from gpi import _lib as L
    lib = L.lib()
    W = {}
    for c in H.layout_cases(layout):
        form = lib.gpi_head_form(C.byref(c.desc(L, 4096, L.HEAD_VALU if valu else 0)), prefetch)
        want = 0 if valu else (c.form if expect_form is None else expect_form)
        assert form == want, (c.id, form, want)
        errs = check_case(c, Runner(c, dev), valu)
        for k, (e, key) in H.worst(errs).items():
            if k not in W or e > W[k][0]:
                W[k] = (e, key, c.id)
    return W


def report(tag, W):
    print('HEADOPS %s ' % tag + ' '.join('%s=%.2e(%s@%s)' % ((k,) + W[k]) for k in sorted(W)))


@pytest.mark.parametrize('form', ['default', 'valu'])
@pytest.mark.parametrize('layout', list(H.LAYOUTS))
def test_head_ops_vs_fp64(device, layout, form):
    """The 26 cases of one layout in one kernel form (module docstring)."""
    W = sweep(layout, form == 'valu', device)
    assert set(W) == {'out', 'terms', 'grad'}
    report('%s form=%s' % (layout, 0 if form == 'valu' else H.LAYOUTS[layout][2]), W)


def test_table_reaches_every_form(device):
    """gpi_head_form over the table under default dispatch: all four forms, each the table's."""
    from gpi import _lib as L
    lib = L.lib()
    seen = {}
    for c in H.cases():
        f = lib.gpi_head_form(C.byref(c.desc(L, 4096)), 1)
        assert f == c.form, c.id
        seen[f] = seen.get(f, 0) + 1
    assert sorted(seen) == [0, 1, 2, 3] and min(seen.values()) >= 10, seen


def run_gemm(g, valu, dev):
    from gpi import _lib as L
    lib = L.lib()
    ws = torch.from_numpy(g.ws).to(dev)
    gacc = torch.zeros(g.n_gacc, dtype=torch.float64, device=dev)
    items = g.gemm_items(L, valu)
    L.check(lib.gpi_outer_gemm(items, len(items), L.ptr(ws), L.ptr(gacc), L.stream_handle()), 'outer gemm')
    torch.cuda.synchronize()
    assert (ws.cpu().numpy().view(np.uint32) == g.ws.view(np.uint32)).all()
    return gacc.cpu().numpy()


@pytest.mark.parametrize('form', ['mfma', 'valu'])
def test_outer_gemm_vs_fp64(device, form):
    """Bare gpi_outer_gemm: S in {1, 3, 17, 67, 130} x (M, N) in {(16,16), (20,36), (5,1), (44,20)}, with and without
    the bias column and the ReLU-on-B flag, strided rows, and one launch of four mixed items: every C and bias block
    within 5e-5 of fp64, nothing written outside them (no bias block without a bias offset)."""
    worst = (0.0, None)
    for g in H.gemm_cases():
        got, ref = run_gemm(g, form == 'valu', device), g.reference()
        mask = np.zeros(g.n_gacc, dtype=bool)
        for k, it in enumerate(g.items):
            blocks = [g.g_reg['c%d' % k]] + ([g.g_reg['bias%d' % k]] if it['bias'] else [])
            for r in blocks:
                e = R.rel_err(r.view(got), r.view(ref))
                assert e <= H.BAR['grad'], (g.id, form, k, e)
                worst = max(worst, (e, g.id))
                mask[r.off:r.off + r.size] = True
        assert (got[~mask] == 0).all(), (g.id, form)
    print('HEADOPS outer_gemm form=%s grad=%.2e(%s)' % ((form,) + worst))


CHILD = '''
import sys
for p in (%r, %r, %r):
    sys.path.insert(0, p)
import torch
import test_gpu_head_ops as T
getattr(T, sys.argv[1])(torch.device('cuda:0'))
'''


def child_generic(dev):
    """GPI_HEAD_PREFETCH=0: the family layouts run the generic MFMA form."""
    assert os.environ.get('GPI_HEAD_PREFETCH') == '0'
    for layout in H.FAMILY_LAYOUTS:
        report('%s form=1 (GPI_HEAD_PREFETCH=0)' % layout, sweep(layout, False, dev, expect_form=1, prefetch=0))


def child_mfma_off(dev):
    """GPI_HEAD_MFMA=0: default dispatch is the VALU form, bit for bit."""
    assert os.environ.get('GPI_HEAD_MFMA') == '0'
    n = 0
    for layout in ('w64_16_64_32', 'w36_20_24_44'):
        for c in H.layout_cases(layout):
            rn = Runner(c, dev)
            a, b = rn.run(False), rn.run(True)
            for x, y in zip(a, b):
                assert (x.view(np.uint64 if x.dtype == np.float64 else np.uint32) ==
                        y.view(np.uint64 if y.dtype == np.float64 else np.uint32)).all(), c.id
            assert not H.over_bar(H.compare(c.extract(*a), c.reference())), c.id
            n += 1
    print('HEADOPS GPI_HEAD_MFMA=0: %d cases bit-equal to GPI_HEAD_VALU' % n)


def run_child(name, env_set):
    env = {k: v for k, v in os.environ.items() if k not in ('GPI_HEAD_PREFETCH', 'GPI_HEAD_MFMA')}
    env.update(env_set)
    r = subprocess.run([sys.executable, '-c', CHILD % (TESTS, ROOT, PKG), name], env=env, capture_output=True,
                       text=True, timeout=240)
    assert r.returncode == 0, (name, r.stdout[-2000:], r.stderr[-3000:])
    print(r.stdout.strip())
    assert 'HEADOPS' in r.stdout


def test_generic_mfma_on_family_widths(device):
    """80/64/64/128 and 64/16/64/32 through head_fwd_mfma / head_bwd_mfma (GPI_HEAD_PREFETCH=0, read once per
    process: a child process), the same comparisons as above."""
    run_child('child_generic', {'GPI_HEAD_PREFETCH': '0'})


def test_mfma_switch_off_equals_valu_flag(device):
    """GPI_HEAD_MFMA=0 (a child process): default dispatch then runs the kernels GPI_HEAD_VALU selects -- workspace,
    terms and accumulator bit-equal -- and they meet the fp64 bars."""
    run_child('child_mfma_off', {'GPI_HEAD_MFMA': '0'})
