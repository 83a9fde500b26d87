"""The yardstick of gpi_rom_fit at nc = 16, without a GPU: the sparse-stiffness restatement
(tests/romfit16_ref.py) is romfit_ref.fit, and the reduced form the kernel evaluates
(u^T G u - 2 b^T u + c with the 7-point G = W^T W) is |W u - Y|^2 on the 16 x 16 coarse mesh."""
import numpy as np
import pytest
import torch

from elbo_ref import physics, tensor_rel
from oracle import fem
import romfit16_ref as R16
import romfit_ref as R


def labels(nc, r, N, seed):
    """Labels with a ROM signal under the noise, as the GPU tests use them: on pure noise some gradients fall
    within Adam's eps, where x carries the last bits of the stiffness sums' order (2e-12 at nc = 16)."""
    return R16.synthetic_labels(nc, r, N, seed, 0.3)


@pytest.mark.parametrize('nc,r,N,T', [(4, 2, 3, 10), (16, 1, 2, 2)])
def test_sparse_restatement_equals_the_dense_one(nc, r, N, T):
    M, W, bc = physics(nc, r)
    Y, F = labels(nc, r, N, seed=7)
    marks = (1, T)
    dense = R.fit(W, M, bc, Y, F, T, 1e-2, marks=marks)
    sparse = R16.fit(W, M, bc, Y, F, T, 1e-2, marks=marks)
    assert set(dense) == set(sparse) and set(sparse['x_marks']) == set(marks)
    errs = {k: tensor_rel(sparse[k], dense[k]) for k in ('x', 'objective', 'sumsq', 'x_eval', 'Y_predict', 'ynorm2')}
    errs['x_marks'] = R.x_drift(sparse['x_marks'], dense['x_marks'])
    print('sparse vs dense restatement, nc = %d: %s' % (nc, errs))
    assert max(errs.values()) < 1e-12, errs
    assert sparse['relerr_list'] == dense['relerr_list'] == []


def test_reduced_residual_and_sparse_gram_matrix_at_nc16():
    nc, r = 16, 2
    W = fem.prolongation_free(fem.unit_square_mesh(nc), fem.unit_square_mesh(nc * r))
    assert W.shape == (1023, 289)
    G = W.T @ W
    nz = np.abs(G) > 1e-14 * np.abs(G).max()
    assert nz.sum(1).max() <= 7 and nz.sum(1).min() >= 1
    p, q = np.nonzero(nz)
    assert set(np.unique(np.abs(p - q))) <= {0, 1, nc + 1, nc + 2}
    rng = np.random.default_rng(3)
    u, Y = rng.standard_normal((4, 289)), 0.3 * rng.standard_normal((4, 1023))
    direct = ((u @ W.T - Y) ** 2).sum(1)
    b, c = Y @ W, (Y ** 2).sum(1)
    reduced = np.einsum('ni,ij,nj->n', u, np.where(nz, G, 0.0), u) - 2 * (b * u).sum(1) + c
    assert tensor_rel(reduced, direct) < 1e-12


def test_sparse_restatement_takes_any_dtype():
    M, W, bc = physics(4, 2)
    Y, F = labels(4, 2, 3, seed=9)
    lo = R16.fit(W, M, bc, Y, F, 3, 1e-2, dtype=torch.float32, marks=(3,))
    hi = R16.fit(W, M, bc, Y, F, 3, 1e-2, marks=(3,))
    assert lo['x'].dtype == np.float32 and hi['x'].dtype == np.float64
    assert R.j_drift(lo['objective'], hi['objective']) < 1e-5
