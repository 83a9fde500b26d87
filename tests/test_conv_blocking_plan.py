"""Host-side guard of tests/test_gpu_conv_blocking.py: planned without a device (gpi_conv_shape_plan), every case
of that file reaches the forward's row-pair form (conv.hip fwd_rows2, ShapeC::npxk = NPX_ROWS2) on a 256-pixel
tile by default and the one-pixel form with GPI_FWD_ROWS2=0, with half tiles where the case is meant to have
them.  The tuning variables are read once per process, so each arm plans in a child process."""
import json
import os
import subprocess
import sys

from conftest import ROOT, PKG

TESTS = os.path.dirname(os.path.abspath(__file__))

CHILD = r'''
import json, sys
sys.path[:0] = [%r, %r, %r]
import test_gpu_conv_blocking as tb
from conv_cases import lay_out, plan_ctx, plan_shape, shape_fields
from gpi import _lib as L
out = {}
for case, _ in tb.FWD_CASES:
    prog = tb.chain_for(case)
    ws, g, descs = lay_out(case, prog)
    rc, s = plan_shape(L.lib(), descs[prog.ops.index(prog.T)], plan_ctx(g), 1, 0, shape_fields())
    assert rc == 0, case.id
    out[case.id] = [s['npxk'], s['half'], s['G_th'] * s['D_w_out'], s['cp'], s['D_in_bn'], s['drop']]
print(json.dumps(out))
''' % (TESTS, ROOT, PKG)


def plan(flag):
    env = dict(os.environ, GPI_FWD_ROWS2=flag, GPI_TILE_FWDUP32='8')
    r = subprocess.run([sys.executable, '-c', CHILD], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_blocking_cases_reach_both_forms():
    from test_gpu_conv_blocking import FWD_CASES, NPX_ROWS2
    on, off = plan('1'), plan('0')
    for case, half in FWD_CASES:
        a, b = on[case.id], off[case.id]
        assert a[0] == NPX_ROWS2 and b[0] == 1, (case.id, a, b)
        assert a[1:] == b[1:] and a[1] == half and a[2] == 256, (case.id, a, b)
        assert a[4] == (0 if getattr(case, 'no_bn', False) else 1) and a[5] == int(case.drop), (case.id, a)
    # the shapes the sweep is for: both accumulator widths of an odd / padded split, and the 2 + 2 one
    assert {v[3] for v in on.values()} == {4, 6, 8}
