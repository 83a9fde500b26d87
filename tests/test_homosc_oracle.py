"""CPU checks of the homoscedastic decoder path (HomoscedasticCNNDecoder, built by ModelFactory(homoscedastic=True):
one mean channel and a learned log-sigma plane shared by every sample): the fp64 oracle (tests/homosc_ref.py)
reproduces the reference runs of tests/golden/elbo_homosc_c32.npz for both settings of reconstruct_log_eff_property, the decoder / factory construct
with the reference's state-dict layout, the plane rides in the shared segment of the flat parameters, the rows of
tests/conv_cases_homosc.py plan onto the tile forms they are chosen for with the fused launch's loss form recorded,
and the launch checks refuse what include/gpi.h says they refuse.  No GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

from gpi import _lib as L
import conv_cases as cc
import conv_cases_homosc as ch
from elbo_ref import load
from homosc_ref import oracle_homosc_fixture_elbo, homosc_vo_fixture, oracle_homosc_vo_fixture_elbo

GPI_ERR_ARG, GPI_ERR_UNSUPPORTED = -1, -3


def test_fixture_holds_both_runs_on_one_state():
    d = load('elbo_homosc_c32.npz')
    assert d['state.f.logsigma'].shape == (32, 32) and np.abs(d['state.f.logsigma'] + 1.0).max() < 2.0
    assert d['state.f.features.LastTransUp.conv3.weight'].shape[0] == 1
    for tag in ('log', 'exp'):
        assert np.abs(d[tag + '.grad.f.logsigma']).max() > 0
    assert float(d['log.elbo']) != float(d['exp.elbo'])


@pytest.mark.parametrize('tag', ['log', 'exp'])
def test_oracle_matches_reference_run(tag):
    """ELBO rtol 2e-5, the two decoder log-likelihoods and every logged term rtol 2e-5, every gradient 2e-4 of
    max(|ref|, 1): test_binary_oracle.py's bars."""
    d = load('elbo_homosc_c32.npz')
    terms = {}
    val, grads = oracle_homosc_fixture_elbo(d, log_field=tag == 'log', terms=terms)
    np.testing.assert_allclose([terms['logl_u'], terms['logl_s']], d[tag + '.logl_field'], rtol=2e-5)
    np.testing.assert_allclose(val, float(d[tag + '.elbo']), rtol=2e-5)
    pre = tag + '.term.objective/'
    keys = [k[len(pre):] for k in d if k.startswith(pre) and not k.endswith('_elbo')]
    assert len(keys) == 7, keys
    for k in keys:
        np.testing.assert_allclose(terms[k], float(d[pre + k]), rtol=2e-5, err_msg=k)
    keys = [k[len(tag) + 6:] for k in d if k.startswith(tag + '.grad.')]
    assert sorted(keys) == sorted(grads) and 'f.logsigma' in keys
    for k in keys:
        ref = d['%s.grad.%s' % (tag, k)]
        scale = max(np.abs(ref).max(), 1.0)
        np.testing.assert_allclose(grads[k] / scale, ref / scale, atol=2e-4, err_msg=k)


def test_plane_gradient_is_the_batch_sum_of_the_per_pixel_terms():
    """The oracle's f.logsigma gradient restated by hand from the two decoder calls' means: sum over the samples
    of 1 - r^2 exp(-2 ls) (the form the epilogue stores per sample and gpi_wgrad_reduce sums)."""
    from homosc_ref import homosc_decoder, _dec_params
    from elbo_ref import CODEC, state_of
    from oracle import codec as ocodec, elbo as oelbo
    d = load('elbo_homosc_c32.npz')
    _, grads = oracle_homosc_fixture_elbo(d)
    st = state_of(d)
    t = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64)
    cfg = CODEC[32]
    enc_p = {k[8:]: v for k, v in st.items() if k.startswith('encoder.')}
    Xu = t(d['Xu'])[torch.as_tensor(d['perm'][:8])]
    mean, ls = ocodec.encoder_forward(enc_p, Xu, 32, cfg['blocks'], cfg['growth'], cfg['f0'])
    dec = homosc_decoder(_dec_params(st), cfg)
    plane = st['f.logsigma'].detach()
    g = torch.zeros_like(plane)
    with torch.no_grad():
        for X, z in ((Xu, oelbo.reparam(mean, ls, t(d['eps_enc']))),
                     (t(d['Xs']), oelbo.reparam(st['q_z.supervised._mean'], st['q_z.supervised._logsigma'],
                                                t(d['eps_qz'])))):
            r = X - dec(z)[0]
            g += (1.0 - r * r * torch.exp(-2.0 * plane)).sum(0)
    np.testing.assert_allclose(grads['f.logsigma'], g.numpy(), rtol=1e-10, atol=1e-10)


def test_homoscedastic_decoder_state_dict_and_factory():
    from bottleneck.Decoder import CNNDecoder, HomoscedasticCNNDecoder
    from factories.model import ModelFactory
    d = load('elbo_homosc_c32.npz')
    mf = ModelFactory.FromIdentifier('highres32', homoscedastic=True, device='cpu')
    assert mf.params['homoscedastic'] is True
    _, model, _, _, _, _ = mf.setup()
    dec = model.f
    assert isinstance(dec, HomoscedasticCNNDecoder) and isinstance(dec, CNNDecoder)
    assert dec._homoscedastic and not dec._binary and dec.native_config()['out_channels'] == 1
    # keys and ORDER as the reference's (the plane is registered before latent_map: the first key)
    assert list(dec.state_dict()) == [k[2:] for k in d['state_keys_f']]
    assert [n for n, _ in dec.named_parameters()][0] == 'logsigma'
    got = {k: tuple(v.shape) for k, v in dec.state_dict().items()}
    assert got == {k[8:]: tuple(v.shape) for k, v in d.items() if k.startswith('state.f.')}
    assert tuple(dec.logsigma.shape) == (32, 32) and not dec.logsigma.detach().any()
    assert tuple(dec.features.LastTransUp.conv3.weight.shape) == (1, 2, 5, 5)
    # the plane is a shared parameter: inside the data-parallel all-reduce bucket of the flat buffer
    flat = model.native_flat()
    assert 0 <= flat.name_offsets['f.logsigma'] and flat.name_offsets['f.logsigma'] + 32 * 32 <= flat.n_shared
    assert flat.name_offsets['f.logsigma'] % 4 == 0
    # built directly: the same layout (the factory's is this class)
    direct = HomoscedasticCNNDecoder(32, 16, (8, 8), 1, 4, [1, 1], False, 4, drop_rate=0.)
    assert list(direct.state_dict()) == list(dec.state_dict()) and direct._homoscedastic
    # force_single_output still has no ELBO; a plain CNNDecoder keeps refusing homoscedastic=True and names the
    # class that builds it; binary wins over homoscedastic (no plane, the Bernoulli head)
    for cls in (CNNDecoder, HomoscedasticCNNDecoder):
        with pytest.raises(NotImplementedError, match='force_single_output'):
            cls(32, 16, (8, 8), 1, 4, [1, 1], False, 4, force_single_output=True)
    with pytest.raises(NotImplementedError, match='HomoscedasticCNNDecoder'):
        CNNDecoder(32, 16, (8, 8), 1, 4, [1, 1], False, 4, homoscedastic=True)
    with pytest.raises(ValueError):
        HomoscedasticCNNDecoder(32, 16, (8, 8), 1, 4, [1, 1], False, 4, homoscedastic=False)
    both = HomoscedasticCNNDecoder(32, 16, (8, 8), 1, 4, [1, 1], True, 4)
    assert both._binary and not both._homoscedastic and not hasattr(both, 'logsigma')
    assert isinstance(both.features.Sigmoid, torch.nn.Sigmoid)
    # the default decoder is unchanged
    plain = CNNDecoder(32, 16, (8, 8), 1, 4, [1, 1], False, 4)
    assert not plain._homoscedastic and plain.native_config()['out_channels'] == 2 and not hasattr(plain, 'logsigma')


def test_codec_ctx_defaults_to_no_plane():
    ctx = L.CodecCtx()
    assert ctx.ls_off == -1 and ctx.gls_off == -1
    assert (L.EPI_GAUSS_HOMO_LOSS, L.EPI_GAUSS_HOMO_EXP_LOSS) == (5, 6)
    assert L.CodecCtx(ls_off=7).ls_off == 7


def _plan(case, chain, ls_off=None):
    lib = L.lib()
    fields = cc.shape_fields()
    prog = chain(case)
    ws, g, descs = cc.lay_out(case, prog)
    ctx = cc.plan_ctx(g)
    if ls_off is not None:
        ctx.ls_off = ls_off
    d = descs[prog.ops.index(prog.T)]
    out = {}
    for what, fwd, fuse in (('fwd', 1, 0), ('bwd', 0, 0), ('fuse', 0, 1)):
        if fuse:
            d.out_off = -1
        rc, s = cc.plan_shape(lib, d, ctx, fwd, fuse, fields)
        assert rc == 0, (case.id, what, rc)
        out[what] = s
    return out


@pytest.mark.parametrize('case', ch.CASES, ids=[c.id for c in ch.CASES])
def test_rows_plan_as_their_gaussian_twins(case):
    """Host side: each row plans, its fused launch is the homoscedastic form (exf 3: log field, 4: exponentiated)
    of a one-channel op, and every launch takes the tile geometry (half tiles, rows per tile) of the Gaussian row
    it mirrors -- with it the tile form that row is in the table for."""
    got, twin = _plan(case, ch.chain, ls_off=0), _plan(ch.gauss_twin(case), cc.chain)
    assert got['fuse']['exf'] == (4 if case.exp_field else 3)
    assert got['fuse']['fusek'] == 1 and got['fuse']['D_cout'] == 1
    assert got['fuse']['D_epilogue'] == ch.epilogue_of(case)
    assert twin['fuse']['exf'] in (0, 1)
    for what in ('fwd', 'bwd', 'fuse'):
        for k in ('half', 'G_th', 'G_tiles', 'G_npx'):
            assert got[what][k] == twin[what][k], (case.id, what, k, got[what][k], twin[what][k])
        for k, v in ch.gauss_twin(case).reach.get(what, {}).items():
            key = k if k in got[what] else 'G_' + k
            assert got[what][key] == v, (case.id, what, k, got[what][key], v)
    table = set(cc.parse_shapes(open(cc.CONV_SHAPES_H).read()))
    assert all(s['_row'] not in table for s in got.values()), 'the rows run the generic kernels'


def test_tile_forms_of_the_rows():
    """What the table is for: one tile per sample at 8^2 and 16^2, several (half tiles among them) at 64^2."""
    by_h = {c.h: _plan(c, ch.chain, ls_off=0) for c in ch.CASES[:4]}
    assert by_h[8]['fuse']['G_tiles'] == 1 and by_h[16]['fuse']['G_tiles'] == 1
    assert by_h[64]['fuse']['G_tiles'] > 1 and by_h[64]['fuse']['half'] == 1
    assert by_h[32]['fwd']['G_th'] == 8


def test_homoscedastic_epilogue_argument_checks():
    """cout = 2, a BN-backward output gradient or no plane (ls_off < 0) with the new epilogues: GPI_ERR_ARG in
    every launch form; a 3x3 op: GPI_ERR_UNSUPPORTED."""
    lib = L.lib()
    for case in (ch.CASES[0], ch.CASES[4]):
        prog = ch.chain(case)
        ws, g, descs = cc.lay_out(case, prog)
        ctx = cc.plan_ctx(g)
        ctx.ls_off = 0
        forms = ((1, 0), (0, 0), (0, 1))
        plan = lambda d, c=ctx: [lib.gpi_conv_shape_plan(C.byref(d), C.byref(c), fwd, fuse) for fwd, fuse in forms]
        d = L.ConvDesc.from_buffer_copy(descs[prog.ops.index(prog.T)])
        assert plan(d) == [0, 0, 0]
        d.cout = 2
        assert plan(d) == [GPI_ERR_ARG] * 3
        d.cout, d.gout_mode = 1, 0
        assert plan(d)[0] == GPI_ERR_ARG
        d.gout_mode = 1
        none = cc.plan_ctx(g)
        assert none.ls_off == -1
        assert plan(d, none) == [GPI_ERR_ARG] * 3
        d.k, d.pad = 3, 1
        assert plan(d) == [GPI_ERR_UNSUPPORTED] * 3


def test_vo_oracle_on_the_homoscedastic_vo_case():
    """homosc_ref.oracle_homosc_vo_fixture_elbo (what the GPU VO test compares the kernels with) runs on the
    homoscedastic form of vo_elbo_c32.npz, active and held off: finite values, the VO rows' gradients present for
    all N_vo = 4 samples, the plane's gradient present, q_X['vo'] reached only by the active term."""
    d = homosc_vo_fixture(load('vo_elbo_c32.npz'))
    assert d['state.f.features.LastTransUp.conv3.weight'].shape[0] == 1 and d['state.f.logsigma'].shape == (32, 32)
    out = {}
    for holdoff in (False, True):
        terms = {}
        vm, vv = (np.concatenate([d[k], d[k][:1]]) for k in ('upd1.mean', 'upd1.vars'))     # a posterior of 4 rows
        val, gr = oracle_homosc_vo_fixture_elbo(d, vm, vv, holdoff=holdoff, terms=terms)
        assert gr['q_z.vo._mean'].shape[0] == 4 and np.abs(gr['q_z.vo._mean'][3]).max() > 0
        assert np.isfinite(val) and np.abs(gr['f.logsigma']).max() > 0
        out[holdoff] = (val, gr, terms)
    assert out[False][0] != out[True][0]
    assert 'q_X.vo._mean' in out[False][1] and 'q_X.vo._mean' not in out[True][1]
