"""Partially observed labels without a GPU: the fp64 restatement (tests/partial_ref.py) reproduces the
reference's own runs with a column-selecting label hook (elbo_partial_c32.npz, romfit_partial_c32.npz,
tests/golden/make_golden_partial.py), and the Python surface -- ObservedDofs, set_label_mask, the descriptors'
new fields -- behaves as documented."""
import numpy as np
import pytest
import torch

from elbo_ref import load, physics, tensor_rel
import partial_ref as P
import romfit_ref as R


# ---------------------------------------------------------------- fixtures against the restatement
def test_elbo_restatement_reproduces_the_reference_run():
    """ELBO rtol 2e-5, the logged labelled terms rtol 2e-5, every gradient 2e-4 of max(|ref|, 1)
    (test_oracle_golden.py's bars)."""
    d = load('elbo_partial_c32.npz')
    idx = d['idx']
    assert idx.shape == (128,) and len(np.unique(idx)) == 128 and idx.max() < 1023
    terms = {}
    val, grads = P.oracle_partial_fixture_elbo(d, P.index_weights(idx, 1023), terms=terms)
    np.testing.assert_allclose(val, float(d['elbo']), rtol=2e-5)
    for k in ('supervised_logL_y', 'supervised_logL_X', 'supervised_logL_x'):
        np.testing.assert_allclose(terms[k], float(d['term.objective/' + k]), rtol=2e-5, err_msg=k)
    keys = [k[5:] for k in d if k.startswith('grad.')]
    assert sorted(keys) == sorted(grads)
    for k in keys:
        ref = d['grad.' + k]
        scale = max(np.abs(ref).max(), 1.0)
        np.testing.assert_allclose(grads[k] / scale, ref / scale, atol=2e-4, err_msg=k)
    # nodes no labelled sample observes: no gradient to logsigma_y, in the reference and in the restatement
    hole = np.setdiff1d(np.arange(1023), idx)
    assert np.all(d['grad.g.logsigmas_y'][hole] == 0) and np.all(grads['g.logsigmas_y'][hole] == 0)
    # ... and the mask matters: the fully observed ELBO is another number
    full, _ = P.oracle_partial_fixture_elbo(d, None)
    assert abs(full - val) > 1e-3 * abs(val)


def test_weighted_likelihood_is_the_column_selected_one():
    gen = torch.Generator().manual_seed(11)
    Y, mu = torch.randn(3, 40, generator=gen, dtype=torch.float64), torch.randn(3, 40, generator=gen, dtype=torch.float64)
    lv = 0.3 * torch.randn(3, 40, generator=gen, dtype=torch.float64)
    idx = np.array([0, 7, 8, 21, 39])
    from oracle import elbo as oelbo
    ref = oelbo.dgll(Y[:, idx], mu[:, idx], lv[:, idx]).item()
    w = P.index_weights(idx, 40)
    np.testing.assert_allclose(P.dgll_weighted(Y, mu, lv, w).item(), ref, rtol=1e-14)
    np.testing.assert_allclose(P.dgll_weighted(Y, mu, lv, np.ones(40)).item(), oelbo.dgll(Y, mu, lv).item(), rtol=1e-14)
    Yn = Y.clone()
    Yn[:, np.setdiff1d(np.arange(40), idx)] = float('nan')       # holes are never read
    assert P.dgll_weighted(Yn, mu, lv, w).item() == P.dgll_weighted(Y, mu, lv, w).item()
    mu_g = mu.clone().requires_grad_(True)
    P.dgll_weighted(Yn, mu_g, lv, w).backward()
    assert torch.isfinite(mu_g.grad).all() and (mu_g.grad[:, 1] == 0).all()


def test_fit_restatement_reproduces_the_reference_run():
    """The bar of test_romfit_oracle.py: 2e-5 on x, the prediction, the objective history and the logged errors."""
    d, g = load('rom_c32.npz'), load('romfit_partial_c32.npz')
    M, W, bc = physics(4, 8)
    T, idx = int(g['T']), g['idx']
    assert len(idx) == 17 * 16                                     # every second free node in both directions
    r = P.fit_index(W, M, bc, d['Y'], d['F'], idx, T, float(g['lr']))
    assert len(g['objective']) == T == len(r['objective'])
    errs = dict(x=tensor_rel(g['logX'], r['x']), Y_predict=tensor_rel(g['Y_predict'], r['Y_predict']),
                objective=R.j_drift(g['objective'], r['objective']),
                relerr=tensor_rel(g['relerr_list'], r['relerr_list']))
    print('reference fp32 run vs fp64 restatement (sensor grid):', errs)
    assert max(errs.values()) < 2e-5, errs
    # the weighted form of the same objective follows the same fp64 trajectory
    w = P.fit_weighted(W, M, bc, d['Y'], d['F'], P.index_weights(idx, W.shape[0]), 20, float(g['lr']), marks=(1, 10, 20))
    i = P.fit_index(W, M, bc, d['Y'], d['F'], idx, 20, float(g['lr']), marks=(1, 10, 20))
    assert R.x_drift(w['x_marks'], i['x_marks']) < 1e-10 and R.j_drift(w['objective'], i['objective']) < 1e-10


# ---------------------------------------------------------------- the Python surface
def test_observed_dofs_is_the_reference_hook():
    from bottleneck.utils import ObservedDofs
    idx = [5, 0, 3]
    o = ObservedDofs(idx)
    y = torch.arange(24.).reshape(2, 2, 6)
    assert torch.equal(o(y), y[..., torch.tensor(idx)])
    assert torch.equal(o.index, torch.tensor(idx)) and len(o) == 3
    w = o.weights(6, 'cpu')
    assert w.dtype == torch.float32 and w.tolist() == [1, 0, 0, 1, 0, 1]
    assert o.weights(6, 'cpu') is w                                # cached: descriptors hold its address
    with pytest.raises(ValueError):
        o.weights(5, 'cpu')
    with pytest.raises(ValueError):
        ObservedDofs([1, 1])


def _cpu_model(n_s=2):
    from bottleneck.Encoder import CNNEncoder
    from bottleneck.Decoder import CNNDecoder
    from bottleneck.components import EffectivePropertyMap, ReducedOrderModelOperator
    from bottleneck.ROM import ROM
    from bottleneck.generative import GenerativeModel
    from physics.grid import StructuredGrid

    class DS(object):
        N = n_s

        def __init__(self, **kw):
            self.kw = kw

        def get(self, k, **_):
            return self.kw[k]

    nc, n, dz = 4, 32, 16
    _, W, _ = physics(nc, n // nc)
    g = ReducedOrderModelOperator(ROM(StructuredGrid(nc), n // nc), torch.tensor(W, dtype=torch.float32),
                                  dtype=torch.float32, device='cpu')
    gp = EffectivePropertyMap(dz, 2 * nc * nc, independent_X=True, dtype=torch.float32, device='cpu')
    dec = CNNDecoder(n, dz, (8, 8), 1, 4, [1, 1], False, 4, drop_rate=0.)
    model = GenerativeModel(f=dec, g=g, gp=gp, dtype=torch.float32, device=torch.device('cpu'))
    model.encoder = CNNEncoder(n, dz, [1, 1], 4, 4, drop_rate=0)
    model.register_supervised_data(DS(X=torch.zeros(n_s, n, n), Y=torch.zeros(n_s, 1023), F_ROM_BC=torch.zeros(n_s, 25)))
    return model


def test_label_mask_and_hook_exclude_each_other():
    from bottleneck.utils import ObservedDofs
    model = _cpu_model()
    assert model.preprocess_y_fct is None and model.label_weights() is None
    model.preprocess_y_fct = ObservedDofs([1, 2])
    with pytest.raises(ValueError):
        model.set_label_mask(torch.ones(2, 1023))
    assert model.label_weights().shape == (1023,) and model.label_weights().sum() == 2
    model.preprocess_y_fct = None
    with pytest.raises(ValueError):
        model.set_label_mask(torch.ones(3, 1023))                  # not the registered labels' shape
    model.set_label_mask(None)
    assert model.label_weights() is None


def test_any_other_hook_still_raises_in_elbo():
    model = _cpu_model()
    model.preprocess_y_fct = lambda y: y[..., :10]
    with pytest.raises(NotImplementedError, match='preprocess_y_fct is not supported on the native path'):
        model.elbo(step=0, armortized_bs=None)


def test_descriptors_carry_the_weight_fields():
    from gpi import _lib as L
    r, f = L.RomDesc(), L.RomFitDesc()
    assert [n for n, _ in L.RomDesc._fields_][-2:] == ['y_weight', 'yw_stride']
    assert [n for n, _ in L.RomFitDesc._fields_][-3:] == ['y_weight', 'yw_stride', 'n_obs']
    assert r.y_weight is None and r.yw_stride == 0 and f.y_weight is None and f.n_obs == 0.0
    L.lib()                                                        # the struct sizes agree with the library's


def test_rom_rejects_misused_weights_without_a_launch():
    """Argument checks come before any launch: a stride that is neither 0 nor d_y, weights outside LOGLIK."""
    import ctypes as C
    from gpi import _lib as L
    lib, GPI_ERR_ARG = L.lib(), -1                                  # (include/gpi.h)
    buf = (C.c_float * 4096)()
    p = C.cast(buf, C.c_void_p).value

    def desc(mode):
        r = L.RomDesc()
        r.nc, r.refine, r.n, r.mode = 4, 8, 1, mode
        for k in ('x', 'F', 'Y', 'logsig_y', 'gx', 'gls_part', 'dmu', 'mu_y', 'y_weight'):
            setattr(r, k, p)
        r.x_stride = r.gx_stride = 32
        return r

    r = desc(L.ROM_LOGLIK)
    for bad in (1, 1022, 1024, -1023):
        r.yw_stride = bad
        assert lib.gpi_rom(C.byref(r), None) == GPI_ERR_ARG, bad
    for mode in (L.ROM_FORWARD, L.ROM_BACKWARD):
        r = desc(mode)
        assert lib.gpi_rom(C.byref(r), None) == GPI_ERR_ARG, mode
    f = L.RomFitDesc()
    f.nc, f.refine, f.n, f.iters = 4, 8, 1, 1
    f.Y = f.F = f.x = f.y_weight = p
    f.x_stride = 32
    f.yw_stride = 7
    assert lib.gpi_rom_fit(C.byref(f), None) == GPI_ERR_ARG
    f.yw_stride, f.n_obs = 0, -1.0
    assert lib.gpi_rom_fit(C.byref(f), None) == GPI_ERR_ARG
