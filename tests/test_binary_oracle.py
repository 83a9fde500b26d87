"""CPU checks of the binary (two-phase) decoder path: the fp64 oracle (tests/binary_ref.py) reproduces the
reference run of tests/golden/elbo_binary_c32.npz, the logit form equals sigmoid + binary cross-entropy, and
the binary decoder / factory construct with the reference's state-dict layout.  No GPU."""
import numpy as np
import torch

from elbo_ref import load
from binary_ref import LOGIT_MAX, bernoulli_loglik, oracle_binary_fixture_elbo, softplus


def test_fixture_is_two_phase_and_in_range():
    d = load('elbo_binary_c32.npz')
    assert float(d['logit_max']) < LOGIT_MAX
    for key in ('Xu', 'Xs'):
        X = d[key]
        assert set(np.unique(X)) == {np.float32(np.log(1.0)), np.float32(np.log(10.0))}
        for img in X:
            assert img.min() != img.max(), 'every image holds both phases'


def test_oracle_matches_reference_run():
    """ELBO rtol 2e-5, every gradient 2e-4 of max(|ref|, 1): test_oracle_golden.py's bars."""
    d = load('elbo_binary_c32.npz')
    terms = {}
    val, grads = oracle_binary_fixture_elbo(d, terms=terms)
    assert terms['logit_max'] < LOGIT_MAX
    np.testing.assert_allclose([terms['logl_u'], terms['logl_s']], d['logl_field'], rtol=2e-5)
    np.testing.assert_allclose(val, float(d['elbo']), rtol=2e-5)
    # every term of the objective the reference logged (a compensating error between terms would pass the total)
    keys = [k[len('term.objective/'):] for k in d if k.startswith('term.objective/') and not k.endswith('_elbo')]
    assert len(keys) == 7, keys
    for k in keys:
        np.testing.assert_allclose(terms[k], float(d['term.objective/' + k]), rtol=2e-5, err_msg=k)
    keys = [k[5:] for k in d if k.startswith('grad.')]
    assert sorted(keys) == sorted(grads)
    for k in keys:
        ref = d['grad.' + k]
        scale = max(np.abs(ref).max(), 1.0)
        np.testing.assert_allclose(grads[k] / scale, ref / scale, atol=2e-4, err_msg=k)


def test_logit_form_is_sigmoid_bce():
    """-softplus(-a) / -softplus(a) vs torch sigmoid + binary_cross_entropy in fp64 on |a| < 15, value and
    gradient (sigmoid(a) - t)."""
    gen = torch.Generator().manual_seed(3)
    a = ((torch.rand(4, 32, 32, generator=gen, dtype=torch.float64) * 2 - 1) * (LOGIT_MAX - 1e-3)).requires_grad_()
    assert float(a.detach().abs().max()) < LOGIT_MAX
    X = torch.where(torch.rand(4, 32, 32, generator=gen) < 0.4, np.log(10.0), np.log(1.0)).double()
    ll = bernoulli_loglik(X, a)
    g, = torch.autograd.grad(-ll, a)
    t = (X != X.min()).double()
    b = a.detach().clone().requires_grad_()
    ref = -torch.nn.functional.binary_cross_entropy(torch.sigmoid(b), t, reduction='sum')
    gref, = torch.autograd.grad(-ref, b)
    np.testing.assert_allclose(ll.item(), ref.item(), rtol=1e-12)
    np.testing.assert_allclose(g.numpy(), gref.numpy(), rtol=0, atol=1e-12)
    np.testing.assert_allclose(g.numpy(), (torch.sigmoid(a.detach()) - t).numpy(), rtol=0, atol=1e-12)
    # the form stays finite where the fp32 sigmoid saturates
    big = torch.tensor([17.0, -17.0, 60.0, -60.0], dtype=torch.float64)
    np.testing.assert_allclose(softplus(big).numpy(), np.log1p(np.exp(big.numpy())), rtol=1e-12)


def test_binary_decoder_state_dict_and_factory():
    from bottleneck.Decoder import CNNDecoder
    import pytest
    d = load('elbo_binary_c32.npz')
    dec = CNNDecoder(32, 16, (8, 8), 1, 4, [1, 1], True, 4, drop_rate=0.)
    assert dec._binary and dec.native_config()['out_channels'] == 1
    assert isinstance(dec.features.Sigmoid, torch.nn.Sigmoid)
    ref = {k[8:]: v.shape for k, v in d.items() if k.startswith('state.f.')}
    got = {k: tuple(v.shape) for k, v in dec.state_dict().items()}
    assert got == {k: tuple(s) for k, s in ref.items()}
    assert got['features.LastTransUp.conv3.weight'][0] == 1
    with pytest.raises(NotImplementedError):
        dec.propagate_samples(torch.zeros(2, 16))
    for kw in (dict(force_single_output=True), dict(homoscedastic=True)):
        with pytest.raises(NotImplementedError):
            CNNDecoder(32, 16, (8, 8), 1, 4, [1, 1], False, 4, **kw)


def test_factory_constructs_binary_model():
    from factories.model import ModelFactory
    mf = ModelFactory.FromIdentifier('highres32', binary_field=True, device='cpu')
    assert mf.params['binary_field'] is True
    _, model, _, _, _, _ = mf.setup()
    assert model.f._binary and model.f.native_config()['out_channels'] == 1
    assert tuple(model.f.features.LastTransUp.conv3.weight.shape) == (1, 2, 5, 5)
    # direct callers of the likelihood: the non-tuple (probability image) branch, the reference's rule
    a = torch.tensor([[[0.3, -1.2], [2.0, -0.1]]])
    X = torch.tensor([[[0.0, 0.0], [2.3, 2.3]]])
    got = model.random_field_likelihood(torch.sigmoid(a), X)
    np.testing.assert_allclose(got.item(), bernoulli_loglik(X.double(), a.double()).item(), rtol=1e-6)


def test_vo_oracle_on_the_binary_vo_case():
    """binary_ref.oracle_binary_vo_fixture_elbo (what the GPU VO test compares the kernels with) runs on the
    binary form of vo_elbo_c32.npz, active and held off: in-range logits, finite values, the VO rows' gradients
    present for all N_vo = 4 samples, the two values different, q_X['vo'] reached only by the active term."""
    from binary_ref import binary_vo_fixture, oracle_binary_vo_fixture_elbo
    d = binary_vo_fixture(load('vo_elbo_c32.npz'))
    for key in ('Xu', 'Xs', 'Xv'):
        assert set(np.unique(d[key])) == {np.float32(np.log(1.0)), np.float32(np.log(10.0))}
    assert d['state.f.features.LastTransUp.conv3.weight'].shape[0] == 1
    out = {}
    for holdoff in (False, True):
        terms = {}
        vm, vv = (np.concatenate([d[k], d[k][:1]]) for k in ('upd1.mean', 'upd1.vars'))     # a posterior of 4 rows
        val, gr = oracle_binary_vo_fixture_elbo(d, vm, vv, holdoff=holdoff, terms=terms)
        assert gr['q_z.vo._mean'].shape[0] == 4 and np.abs(gr['q_z.vo._mean'][3]).max() > 0
        assert np.isfinite(val) and terms['logit_max'] < LOGIT_MAX
        assert np.abs(gr['q_z.vo._mean']).max() > 0
        out[holdoff] = (val, gr, terms)
    assert out[False][0] != out[True][0]
    assert 'q_X.vo._mean' in out[False][1] and 'q_X.vo._mean' not in out[True][1]
