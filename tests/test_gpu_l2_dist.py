"""The L2 penalty of the fused step under data parallelism: two gloo ranks on the one GPU (tests/dp_worker_l2.py),
each running forward_backward() + the SUM all-reduce once without the penalty and once with it, from the same
seeds.

The shared gradient is summed over the ranks, so the penalty must enter ONCE: every rank adds it to the all-reduced
gradient after the SUM (the Adam launch, which stores the sum back).  Checked on the gradient of the update: on the
shared prefix G_l2 - G_none is lambda p / ||p|| once (the bound of
tests/test_gpu_l2_step.py (a): 4 * 2^-24 (|G_none| + |lambda p / ||p|||)), identically on both ranks; the rank-local
q rows are bit-identical; every rank reports the penalty in terms(); the ranks' elbo() values sum to the sum without
the penalty less lambda * pen, once."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def test_dp_two_ranks_l2_penalty_enters_once(device, tmp_path):
    from test_gpu_dist import _free_port
    from test_gpu_l2_step import penalty_reference, U
    env = dict(os.environ)
    env['PYTHONUNBUFFERED'] = '1'
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node=2',
           '--master-addr=127.0.0.1', '--master-port=%d' % _free_port(), os.path.join(HERE, 'dp_worker_l2.py'),
           str(tmp_path)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    rk = [dict(np.load(str(tmp_path / ('rank%d.npz' % i)))) for i in range(2)]
    lam = float(rk[0]['lam'])
    assert lam == float(rk[1]['lam']) and lam > 0
    ns = int(rk[0]['none.n_shared'])
    rows = [(None, int(o), int(n)) for o, n in rk[0]['none.rows']]
    assert np.array_equal(rk[0]['none.rows'], rk[1]['l2.rows'])
    P0 = rk[0]['none.P0']
    x, mask, pen, norms = penalty_reference(P0, rows, lam)
    assert (norms == 0).any() and (norms > 0).any() and mask[ns:].sum() == 0
    for r_ in rk:
        assert np.array_equal(r_['none.P0'][:ns], P0[:ns]) and np.array_equal(r_['l2.P0'], r_['none.P0'])
        Gn, Gl = r_['none.G_step'], r_['l2.G_step']
        assert np.array_equal(Gn, r_['none.G_red'])
        # rank-local q rows: the penalty never reaches them
        assert np.array_equal(Gn[ns:].view(np.uint32), Gl[ns:].view(np.uint32))
        assert np.array_equal(Gn[:ns][~mask[:ns]].view(np.uint32), Gl[:ns][~mask[:ns]].view(np.uint32))
        err = np.abs(Gl.astype(np.float64) - (Gn.astype(np.float64) + x))[mask]
        bound = (4 * U * (np.abs(Gn.astype(np.float64)) + np.abs(x)))[mask]
        assert (err <= bound).all(), (err[bound > 0] / bound[bound > 0]).max()
        assert not np.array_equal(Gn[mask], Gl[mask])
        assert np.isnan(r_['none.pen']) and abs(float(r_['l2.pen']) - pen) <= 1e-6 * pen
    # the same reduced gradient and the same parameters after Adam on both ranks
    assert np.array_equal(rk[0]['l2.G_step'][:ns], rk[1]['l2.G_step'][:ns])
    assert np.array_equal(rk[0]['l2.P1'][:ns], rk[1]['l2.P1'][:ns])
    assert not np.array_equal(rk[0]['l2.P1'][:ns], rk[0]['none.P1'][:ns])
    # nothing of the penalty goes through the exchange
    for r_ in rk:
        assert np.array_equal(r_['l2.G_local'], r_['none.G_local']) and np.array_equal(r_['l2.G_red'], r_['none.G_red'])
    # the objective: the ranks' values sum to the global ELBO less the penalty, once
    lam32 = float(np.float32(lam))
    s_none = sum(float(r_['none.elbo']) for r_ in rk)
    s_l2 = sum(float(r_['l2.elbo']) for r_ in rk)
    want = s_none - lam32 * pen
    assert abs(s_l2 - want) <= 1e-6 * max(abs(want), abs(s_none)), (s_l2, want)
    assert float(rk[1]['l2.elbo']) == float(rk[1]['none.elbo'])
