"""The segment table of the fused step's L2 penalty (gpi.train.l2_segments) without a GPU or the library: the
rows are the tensors model.elbo(l2_penalty=) penalises -- f.parameters() then encoder.parameters()
(generative.py:381-385) -- at their places in the flat parameter buffer, and nothing else."""
import numpy as np
import torch

from elbo_ref import load


class _DS(object):
    def __init__(self, **t):
        self.t = t
        self.N = next(iter(t.values())).shape[0]

    def __bool__(self):
        return True

    def get(self, key, random_subset=None):
        return self.t[key] if random_subset is None else self.t[key][:random_subset]


def golden_model_cpu(d):
    """tests/test_gpu_parity.py::build_golden_model on the CPU (the layout needs no device)."""
    from bottleneck.Encoder import CNNEncoder
    from bottleneck.Decoder import CNNDecoder
    from bottleneck.components import EffectivePropertyMap, ReducedOrderModelOperator
    from bottleneck.ROM import ROM
    from bottleneck.generative import GenerativeModel
    from physics.grid import StructuredGrid
    n, nc, dz, Nu, bs, Ns = [int(v) for v in d['cfg']]
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32)
    enc = CNNEncoder(n, dz, [1, 1], 4, 4, drop_rate=0)
    dec = CNNDecoder(n, dz, (8, 8), 1, 4, [1, 1], False, 4, drop_rate=0.)
    g = ReducedOrderModelOperator(ROM(StructuredGrid(nc), n // nc), torch.tensor(d['W']), dtype=torch.float32,
                                  device='cpu')
    gp = EffectivePropertyMap(dz, 2 * nc * nc, independent_X=True, dtype=torch.float32, device='cpu')
    model = GenerativeModel(f=dec, g=g, gp=gp, dtype=torch.float32, device=torch.device('cpu'))
    model.encoder = enc
    model.register_datasets({'supervised': _DS(X=t(d['Xs']), Y=t(d['Y']), F_ROM_BC=t(d['F'])),
                             'unsupervised': _DS(X=t(d['Xu']))}, None,
                            create_unsupervised_variational_approximation=False)
    model.load_state_dict({k[6:]: torch.tensor(v) for k, v in d.items() if k.startswith('state.')})
    return model


def homosc_model_cpu():
    from factories.model import ModelFactory
    _, model, _, encoder, _, _ = ModelFactory.FromIdentifier('highres32', homoscedastic=True, device='cpu').setup()
    if getattr(model, 'encoder', None) is None:
        model.encoder = encoder
    return model


def check_rows(model):
    from gpi.train import l2_segments
    flat = model.native_flat()
    rows = l2_segments(model)
    assert rows == l2_segments(model, flat)
    want = ['f.' + n for n, _ in model.f.named_parameters()] + \
           ['encoder.' + n for n, _ in model.encoder.named_parameters()]
    assert [r[0] for r in rows] == want and len(set(want)) == len(want)
    params = dict(model.named_parameters())
    covered = np.zeros(flat.numel, dtype=bool)
    for name, off, numel in rows:
        assert off == flat.name_offsets[name] and numel == params[name].numel() and numel >= 1
        assert 0 <= off and off + numel <= flat.n_shared
        assert not covered[off:off + numel].any(), 'rows overlap'
        covered[off:off + numel] = True
    # nothing else: the error slot, the padding floats and every other parameter stay outside the rows
    assert 0 <= flat.err_slot < flat.n_shared and not covered[flat.err_slot]
    owned = np.zeros(flat.numel, dtype=bool)
    others = [n for n in flat.names if n not in want]
    assert any(n.startswith('gp.') for n in others) and any(n.startswith('g.') for n in others)
    for n in flat.names:
        o = flat.name_offsets[n]
        owned[o:o + params[n].numel()] = True
        if n in others:
            assert n.startswith(('gp.', 'g.', 'q_')), n
            assert not covered[o:o + params[n].numel()].any(), n
    assert not covered[~owned].any()
    assert covered.sum() == sum(p.numel() for p in model.f.parameters()) + \
        sum(p.numel() for p in model.encoder.parameters())
    return rows, flat


def test_rows_of_the_c32_golden_model():
    d = load('elbo_opts_c32.npz')
    model = golden_model_cpu(d)
    rows, flat = check_rows(model)
    names = [r[0] for r in rows]
    assert any(n.startswith('q_') for n in flat.names), 'the model has per-sample rows behind the shared prefix'
    # BN weights and biases, latent_map and the encoder's dense head are penalised tensors of their own
    assert 'f.latent_map.weight' in names and 'f.latent_map.bias' in names
    assert any('norm' in n and n.endswith('.bias') for n in names)
    assert 'encoder.features.SplitDense.fc_logvar.weight' in names
    assert min(r[2] for r in rows) < 64 < max(r[2] for r in rows)


def test_rows_of_a_homoscedastic_model():
    model = homosc_model_cpu()
    rows, flat = check_rows(model)
    by_name = {r[0]: r for r in rows}
    assert by_name['f.logsigma'][2] == 32 * 32
    assert rows[0][0] == 'f.logsigma'           # (registered ahead of latent_map: the decoder's first parameter)
