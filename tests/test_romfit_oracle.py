"""The algebra gpi_rom_fit rests on, and its yardstick, without a GPU (tests/romfit_ref.py):
G = W^T W is 7-point sparse, the reduced form follows the direct form's fp64 trajectory, and the fp64
restatement reproduces the reference's own OptimizeEffectiveProperties run (romfit_c32.npz,
tests/golden/make_golden_romfit.py)."""
import numpy as np
import pytest

from elbo_ref import load, physics, tensor_rel
from oracle import fem
import romfit_ref as R


@pytest.mark.parametrize('nc,r', [(4, 2), (4, 8), (8, 8)])
def test_gram_matrix_has_at_most_seven_nonzeros_per_row(nc, r):
    W = fem.prolongation_free(fem.unit_square_mesh(nc), fem.unit_square_mesh(nc * r))
    G = W.T @ W
    assert G.shape == ((nc + 1) ** 2,) * 2
    nnz = (np.abs(G) > 1e-14 * np.abs(G).max()).sum(1)
    assert nnz.max() <= 7 and nnz.min() >= 1
    # ... and they are the node itself, its +-x, +-y neighbours and the two on the "/" diagonal
    p, q = np.nonzero(np.abs(G) > 1e-14 * np.abs(G).max())
    assert set(np.unique(np.abs(p - q))) <= {0, 1, nc + 1, nc + 2}


def test_reduced_form_follows_the_direct_trajectory():
    d = load('rom_c32.npz')
    M, W, bc = physics(4, 8)
    direct = R.fit(W, M, bc, d['Y'], d['F'], 50, 1e-2, marks=(1, 10, 50))
    reduced = R.fit(W, M, bc, d['Y'], d['F'], 50, 1e-2, reduced=True, marks=(1, 10, 50))
    ex, ej = R.x_drift(reduced['x_marks'], direct['x_marks']), R.j_drift(reduced['objective'], direct['objective'])
    print('reduced vs direct, 50 iterations fp64: x %.2e, J %.2e' % (ex, ej))
    assert ex < 1e-10
    assert ej < 1e-8
    assert tensor_rel(reduced['sumsq'], direct['sumsq']) < 1e-8


def test_restatement_reproduces_the_reference_run():
    d, g = load('rom_c32.npz'), load('romfit_c32.npz')
    M, W, bc = physics(4, 8)
    T = int(g['T'])
    r = R.fit(W, M, bc, d['Y'], d['F'], T, float(g['lr']))
    assert len(g['objective']) == T == len(r['objective'])
    assert len(g['relerr_list']) == len(r['relerr_list']) == 2
    errs = dict(x=tensor_rel(g['logX'], r['x']), Y_predict=tensor_rel(g['Y_predict'], r['Y_predict']),
                objective=R.j_drift(g['objective'], r['objective']),
                relerr=tensor_rel(g['relerr_list'], r['relerr_list']))
    print('reference fp32 run vs fp64 restatement:', errs)
    assert max(errs.values()) < 2e-5, errs
