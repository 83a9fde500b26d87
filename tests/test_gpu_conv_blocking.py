"""Register blocking of the conv forward (conv.hip, NPX_ROWS2 / fwd_rows2): on 3x3 / stride-1 tiles of 256 output
pixels a thread takes two vertically adjacent pixels and one half of the output channels instead of one pixel and
every channel.  Each output still accumulates over (ci, ky, kx) in the same order, so against the one-pixel form
(GPI_FWD_ROWS2=0, a child process of its own, as tests/test_gpu_shapes.py runs GPI_CONV_SHAPES=0) every stored
activation must be equal bit for bit; the BN statistics are held to fp64 sums of the stored values at the project's
1e-6 bar (the form adds them in the one-pixel form's order, which the whole-step test below relies on).  Both arms
also pass the whole per-operator check of tests/test_gpu_conv_ops.py (fp64 reference, its BARS, untouched memory)
inside the child.

Shapes: the smallest at which the form can go wrong -- 16-row tiles of a 16-wide plane and 8-row tiles of a 32-wide
one, an odd channel split (5 = 3 + 2), a padded one (6 outputs on 8 accumulators), no input BN, the upsampling
conv on 256-pixel tiles (GPI_TILE_FWDUP32=8 in both arms), Dropout2d scales, and a batch whose last samples run
half-height tiles.  Batch 3 in two BN groups, except where the half tiles need more than 256 tiles."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, PKG
from conv_cases import Case, chain

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
NPX_ROWS2 = -2          # conv.hip: ShapeC::npxk of the row-pair form


class NoBnCase(Case):
    """T without an input BN (the decoder's first conv): producer -> T -> consumer as conv_cases.chain."""
    no_bn = True

    @property
    def id(self):
        return Case.id.fget(self) + '_nobn'


def chain_for(case):
    """conv_cases.chain, or for a NoBnCase the same chain with T reading its input without BN + ReLU."""
    from gpi.plan import CodecProgram
    if not getattr(case, 'no_bn', False):
        return chain(case)
    P = CodecProgram('conv_case', 0.0)
    h, w = case.h, case.w
    z = P.buf('z', 4, h, w)
    P.input = z
    X = P.buf('X', case.cin, h, w)
    Y = P.buf('Y', case.cout + 1, h, w)
    P.conv('p0', z, 0, 4, X, 0, case.cin, 1, 1, 0, 0, 'p0.weight')
    P.T = P.conv('T', X, 0, case.cin, Y, 0, case.cout, case.k, 1, case.k // 2, 0, 'T.weight')
    out = P.buf('out', 3, h, w)
    P.conv('c', Y, 0, case.cout, out, 0, 3, 1, 1, 0, 0, 'c.weight', bn='c.bn')
    P.output = out
    return P


G3 = [2, 1]
# (case, forward half tiles expected)
FWD_CASES = [
    (Case(3, 's1', 5, 4, 16, 16, G3, grad=False, seed=101), 0),
    (Case(3, 's1', 6, 4, 32, 32, G3, grad=False, seed=102), 0),
    (Case(3, 's1', 10, 5, 32, 32, G3, grad=False, seed=103), 0),
    (NoBnCase(3, 's1', 1, 6, 32, 32, G3, grad=False, seed=104), 0),
    (Case(3, 'up', 6, 6, 16, 16, G3, grad=False, seed=105), 0),
    (Case(3, 's1', 6, 4, 32, 32, G3, grad=False, drop=True, seed=106), 0),
    (Case(3, 's1', 5, 4, 16, 16, [130, 129], grad=False, seed=107), 1),
]
IDS = [c.id for c, _ in FWD_CASES]

CHILD = r'''
import sys
sys.path[:0] = [%r, %r, %r]
import numpy as np, torch
import test_gpu_conv_ops as ops
import test_gpu_conv_blocking as tb
from conv_cases import lay_out, plan_ctx, plan_shape, shape_fields
from gpi import _lib as L

ops.chain = tb.chain_for
dev = torch.device('cuda', 0)
res = {}
for case, _ in tb.FWD_CASES:
    r = ops.run_gpu(case, dev)
    fwd, _, _ = ops.check_run(case, r)
    prog = r['prog']
    ws, g, descs = lay_out(case, prog)
    rc, s = plan_shape(L.lib(), descs[prog.ops.index(prog.T)], plan_ctx(g), 1, 0, shape_fields())
    assert rc == 0, case.id
    Y = prog.T.dst
    res[case.id + '/T'] = np.ascontiguousarray(fwd['T'])
    res[case.id + '/stats'] = r['stats'][:len(case.groups), Y.stat:Y.stat + case.cout, :2]
    res[case.id + '/stat_err'] = np.array(max(v for v, _ in ops.stat_errors(case, r).values()))
    res[case.id + '/form'] = np.array([s['npxk'], s['half'], s['G_th'] * s['D_w_out'], s['cp']])
np.savez(sys.argv[1], **res)
''' % (TESTS, ROOT, PKG)


@pytest.fixture(scope='module')
def arms(device, tmp_path_factory):
    """{'rows2' | 'onepx': results of every case} -- one child process per arm."""
    out = {}
    d = tmp_path_factory.mktemp('blocking')
    for name, flag in (('rows2', '1'), ('onepx', '0')):
        path = str(d / (name + '.npz'))
        env = dict(os.environ, GPI_FWD_ROWS2=flag, GPI_TILE_FWDUP32='8')
        r = subprocess.run([sys.executable, '-c', CHILD, path], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (name, r.stdout[-2000:], r.stderr[-3000:])
        print(r.stdout)
        out[name] = np.load(path)
    return out


def test_bench_step_bit_identical_with_and_without_row_pairs(device, tmp_path):
    """Two eager steps (forward, backward, Adam) of the bench workload with the row-pair form and with the one-pixel
    form: parameters and the last gradient equal bit for bit.  The form's statistics epilogue adds in the one-pixel
    form's order (rows of 16 lanes, then (R3 + R2) + (R1 + R0), then the waves), so the BN statistics -- and every
    launch after them -- keep their bits; a sum in any other order moves the step by rounding that training amplifies."""
    from test_gpu_shapes import STEP
    res = {}
    for name, flag in (('rows2', '1'), ('onepx', '0')):
        out = str(tmp_path / (name + '.npz'))
        r = subprocess.run([sys.executable, '-c', STEP, out], env=dict(os.environ, GPI_FWD_ROWS2=flag),
                           capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, r.stderr[-3000:]
        res[name] = np.load(out)
    for k in ('P', 'G'):
        a, b = res['rows2'][k], res['onepx'][k]
        assert a.shape == b.shape
        diff = np.flatnonzero(a.view(np.uint32) != b.view(np.uint32))
        assert diff.size == 0, (k, diff.size, float(np.abs(a - b).max()))


@pytest.mark.parametrize('case,half', FWD_CASES, ids=IDS)
def test_row_pair_forward_bit_identical_to_one_pixel_form(case, half, arms):
    from test_gpu_conv_ops import BARS
    a, b = arms['rows2'], arms['onepx']
    fa, fb = a[case.id + '/form'], b[case.id + '/form']
    # both arms on 256-pixel tiles of the same accumulator count; the forms under test, half tiles where meant
    assert fa[0] == NPX_ROWS2 and fb[0] == 1, (fa, fb)
    assert fa[1] == fb[1] == half and fa[2] == fb[2] == 256 and fa[3] == fb[3], (fa, fb)
    ta, tb_ = a[case.id + '/T'], b[case.id + '/T']
    assert ta.shape == tb_.shape and ta.dtype == np.float32
    diff = np.flatnonzero(ta.view(np.uint32) != tb_.view(np.uint32))
    assert diff.size == 0, (case.id, diff.size, float(np.abs(ta - tb_).max()))
    # statistics: each arm against fp64 sums of its stored values (computed in the child by stat_errors)
    ea, eb = float(a[case.id + '/stat_err']), float(b[case.id + '/stat_err'])
    print('%s statistics vs fp64 sums: row pairs %.2e, one pixel %.2e' % (case.id, ea, eb))
    assert ea <= BARS['stat'] and eb <= BARS['stat'], (ea, eb)
    # and the two arms' sums of the same stored values agree within twice that bar
    sa, sb = a[case.id + '/stats'], b[case.id + '/stats']
    for k in range(2):
        scale = np.abs(sb[..., k]).max()
        assert np.abs(sa[..., k] - sb[..., k]).max() <= 2 * BARS['stat'] * scale
