"""The fp64 eval-mode restatement (tests/eval_ref.py) against the reference's own eval-mode run
(tests/golden/codec_eval_*.npz, fp32): 1e-5 relative norm.  The reference's fp32 output sits at
<= 1.8e-6 from the restatement on both configurations, so the bound keeps a 5x margin."""
import os

import numpy as np
import pytest

import eval_ref

GOLD = os.path.join(os.path.dirname(__file__), 'golden')


def load(name):
    return dict(np.load(os.path.join(GOLD, name), allow_pickle=False))


@pytest.mark.parametrize('tag', ['c32', 'c64'])
def test_eval_restatement_matches_reference_fixture(tag):
    d = load('codec_eval_%s.npz' % tag)
    assert d['X'].shape[0] == 3 and float(d['p']) == 0.2
    out = eval_ref.fixture_eval(d)
    for k, v in out.items():
        err = eval_ref.relnorm(d[k], v)
        print(tag, k, 'relative norm %.3e' % err)
        assert err < 1e-5, (k, err)


@pytest.mark.parametrize('tag', ['c32', 'c64'])
def test_fixture_running_buffers_differ_between_consumers_of_a_block(tag):
    """The BN layers that read the same dense-block channels hold different running statistics
    (an implementation that shares one record per block channel cannot pass the parity tests)."""
    d = load('codec_eval_%s.npz' % tag)
    a = d['enc.features.EncBlock1.denselayer1.norm1.running_mean']
    b = d['enc.features.TransDown1.norm1.running_mean']
    assert np.abs(a - b[:a.shape[0]]).max() > 0.1
    v = d['enc.features.TransDown1.norm1.running_var']
    assert v.min() >= 0.5 and v.max() < 1.5
