"""CPU checks of the nonlinear effective-property map (hidden layers in gp): the linear-decay widths, the
reference's state-dict layout, the factory option, and the fp64 oracle (tests/gp_mlp_ref.py) against the reference
run of tests/golden/elbo_gpmlp_c32.npz.  No GPU."""
import numpy as np
import pytest
import torch

from elbo_ref import load
from gp_mlp_ref import CASES, FIXTURE, case_of, mlp, mlp_layers, oracle_gpmlp_fixture_elbo

PREACT_MIN = 1e-4     # the generator's bar on every hidden pre-activation of the reference run


@pytest.fixture(scope='module')
def fixture():
    return load(FIXTURE)


@pytest.mark.parametrize('dim_in,dim_out,L,want', [(16, 32, 1, [24]), (16, 32, 2, [21, 26]), (64, 128, 1, [96]),
                                                   (64, 128, 2, [85, 106]), (64, 512, 1, [288]),
                                                   (64, 512, 2, [213, 362])])
def test_linear_decay_widths(dim_in, dim_out, L, want):
    from lamp.neuralnets import FeedforwardNeuralNetwork, linear_decay_widths
    assert linear_decay_widths(dim_in, dim_out, L) == want
    net = FeedforwardNeuralNetwork.FromLinearDecay(dim_in, dim_out, L)
    assert net.widths == [dim_in] + want + [dim_out]
    names = [n for n, _ in net.layers.named_children()]
    assert names == [s for k in range(1, L + 1) for s in ('fc%d' % k, 'activ%d' % k)] + ['fc%d' % (L + 1)]
    assert all(isinstance(net.layers.get_submodule('activ%d' % k), torch.nn.ReLU) for k in range(1, L + 1))
    with pytest.raises(NotImplementedError):
        FeedforwardNeuralNetwork(dim_in, dim_out, want, 0.5)
    with pytest.raises(NotImplementedError):
        FeedforwardNeuralNetwork(dim_in, dim_out, want, None, outf='sigmoid')


def test_state_dict_layout_is_the_reference(fixture):
    """Keys, order and shapes of EffectivePropertyMap(16, 32, num_hidden_layers = 2) equal the reference's
    state.gp.* (logsigmas_X first, then fc.layers.fc1.weight, fc.layers.fc1.bias, ...); lock-X has no logsigmas_X."""
    from bottleneck.components import EffectivePropertyMap
    for tag, L, indep in (('fx2', 2, True), ('fx1', 1, True), ('lx1', 1, False)):
        d = case_of(fixture, tag)
        ref = [(k[len('state.gp.'):], tuple(v.shape)) for k, v in d.items() if k.startswith('state.gp.')]
        gp = EffectivePropertyMap(16, 32, num_hidden_layers=L, independent_X=indep)
        got = [(k, tuple(v.shape)) for k, v in gp.state_dict().items()]
        assert got == ref, (tag, got, ref)
        assert gp.num_hidden_layers == L
    assert [k for k, _ in got] == ['fc.layers.fc1.weight', 'fc.layers.fc1.bias', 'fc.layers.fc2.weight',
                                   'fc.layers.fc2.bias']
    lin = EffectivePropertyMap(16, 32)           # L = 0: the unchanged nn.Linear
    assert isinstance(lin.fc, torch.nn.Linear) and lin.num_hidden_layers == 0
    assert list(lin.state_dict()) == ['logsigmas_X', 'fc.weight', 'fc.bias']


def test_module_forward_is_the_mlp(fixture):
    """forward / forward_mean / propagate_samples / extract_deterministic_map of the module against the helper's
    restatement on the fixture's weights."""
    from bottleneck.components import EffectivePropertyMap
    d = case_of(fixture, 'fx2')
    gp = EffectivePropertyMap(16, 32, num_hidden_layers=2, dtype=torch.float64, device='cpu')
    gp.load_state_dict({k[len('state.gp.'):]: torch.tensor(v, dtype=torch.float64) for k, v in d.items()
                        if k.startswith('state.gp.')})
    z = torch.randn(5, 16, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    st = {k[6:]: torch.tensor(v, dtype=torch.float64) for k, v in d.items() if k.startswith('state.gp.')}
    ref = mlp(mlp_layers(st), z)
    mean, ls = gp(z)
    np.testing.assert_allclose(mean.detach().numpy(), ref.numpy(), rtol=1e-13, atol=1e-13)
    assert ls.shape == mean.shape
    np.testing.assert_allclose(gp.forward_mean(z).detach().numpy(), ref.numpy(), rtol=1e-13, atol=1e-13)
    assert gp.propagate_samples(z).shape == ref.shape
    det = gp.extract_deterministic_map(duplicate=True)
    assert det is not gp.fc and det.layers.fc1.weight.data_ptr() != gp.fc.layers.fc1.weight.data_ptr()
    np.testing.assert_allclose(det(z).detach().numpy(), ref.numpy(), rtol=1e-13, atol=1e-13)


def test_factory_builds_the_mlp_model():
    from factories.model import ModelFactory
    from lamp.neuralnets import FeedforwardNeuralNetwork
    mf = ModelFactory.FromIdentifier('highres32', eff_property_map_hidden_layers=1, device='cpu')
    _, model, disc, _, _, _ = mf.setup()
    assert isinstance(model.gp.fc, FeedforwardNeuralNetwork) and model.gp.fc.widths == [16, 24, 32]
    assert isinstance(disc._gp, FeedforwardNeuralNetwork) and disc._gp.widths == [16, 24, 32]
    assert disc._gp is not model.gp.fc
    for a, b in zip(disc._gp.parameters(), model.gp.fc.parameters()):
        assert a.data_ptr() != b.data_ptr() and torch.equal(a, b)          # a deep copy
    names = [n for n, _ in model.named_parameters() if n.startswith('gp.')]
    assert names == ['gp.logsigmas_X', 'gp.fc.layers.fc1.weight', 'gp.fc.layers.fc1.bias', 'gp.fc.layers.fc2.weight',
                     'gp.fc.layers.fc2.bias']


@pytest.mark.parametrize('tag', CASES)
def test_oracle_matches_reference_run(fixture, tag):
    """ELBO rtol 2e-5, every logged term 2e-5, every gradient 2e-4 of max(|ref|, 1): test_binary_oracle.py's bars."""
    d = case_of(fixture, tag)
    assert float(d['preact_min']) >= PREACT_MIN
    terms = {}
    val, grads = oracle_gpmlp_fixture_elbo(d, terms=terms)
    assert terms['preact_min'] >= PREACT_MIN
    np.testing.assert_allclose(terms['preact_min'], float(d['preact_min']), rtol=1e-3)
    np.testing.assert_allclose(val, float(d['elbo']), rtol=2e-5)
    keys = [k[len('term.objective/'):] for k in d if k.startswith('term.objective/') and not k.endswith('_elbo')]
    assert len(keys) == (7 if int(d['independent_X']) else 5), keys
    for k in keys:
        np.testing.assert_allclose(terms[k], float(d['term.objective/' + k]), rtol=2e-5, err_msg=k)
    keys = [k[5:] for k in d if k.startswith('grad.')]
    assert sorted(keys) == sorted(grads)
    assert sum(k.startswith('gp.fc.layers.') for k in keys) == 2 * (int(d['L']) + 1)
    for k in keys:
        ref = d['grad.' + k]
        scale = max(np.abs(ref).max(), 1.0)
        np.testing.assert_allclose(grads[k] / scale, ref / scale, atol=2e-4, err_msg=k)
