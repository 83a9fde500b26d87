"""The ELBO with the homoscedastic decoder (one mean channel + the learned log-sigma plane f.logsigma) on the GPU:
GenerativeModel.elbo + backward for both settings of reconstruct_log_eff_property, the fused training step (eager
and captured; the plane under Adam), the C64 codec with dropout, the VO term (active / held off), one
PredictionEnsemble update and the training- and eval-mode forward of a HomoscedasticCNNDecoder, against the fp64
oracle (tests/homosc_ref.py, with the kernels' ReLU decisions) and the reference runs of
tests/golden/elbo_homosc_c32.npz."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_gpu_parity import load, cuda, _DS
from test_gpu_c64 import check_mask_audit

pytestmark = pytest.mark.gpu


def homosc_model(d, log_field=True):
    """The fixture's model on the GPU: test_gpu_parity.build_golden_model with the homoscedastic decoder."""
    from bottleneck.Encoder import CNNEncoder
    from bottleneck.Decoder import HomoscedasticCNNDecoder
    from bottleneck.components import EffectivePropertyMap, ReducedOrderModelOperator
    from bottleneck.ROM import ROM
    from bottleneck.generative import GenerativeModel
    from physics.grid import StructuredGrid
    n, nc, dz, Nu, bs, Ns = [int(v) for v in d['cfg']]
    enc = CNNEncoder(n, dz, [1, 1], 4, 4, drop_rate=0)
    dec = HomoscedasticCNNDecoder(n, dz, (8, 8), 1, 4, [1, 1], False, 4, drop_rate=0.)
    rom = ROM(StructuredGrid(nc), n // nc)
    g = ReducedOrderModelOperator(rom, torch.tensor(d['W']), dtype=torch.float32, device='cuda')
    gp = EffectivePropertyMap(dz, 2 * nc * nc, independent_X=True, dtype=torch.float32, device='cuda')
    model = GenerativeModel(f=dec.cuda(), g=g, gp=gp, dtype=torch.float32, device=torch.device('cuda'))
    model.encoder = enc.cuda()
    ds_s = _DS(X=cuda(d['Xs']), Y=cuda(d['Y']), F_ROM_BC=cuda(d['F']))
    ds_u = _DS(perm=torch.tensor(d['perm'], device='cuda'), X=cuda(d['Xu']))
    model.register_datasets({'supervised': ds_s, 'unsupervised': ds_u}, None,
                            create_unsupervised_variational_approximation=False)
    model.load_state_dict({k[6:]: torch.tensor(v) for k, v in d.items() if k.startswith('state.')})
    model.cuda()
    if not log_field:
        model.set('reconstruct_log_eff_property', False)
    return model, bs


@pytest.mark.parametrize('normalize', [False, True], ids=['sum', 'normalize'])
@pytest.mark.parametrize('tag', ['log', 'exp'])
def test_homosc_elbo_module_path_c32(device, tag, normalize):
    """model.elbo + backward on the fixture's inputs and noise: vs the fp64 oracle with the kernels' ReLU decisions
    at 1e-5 (value) and 5e-5 per gradient tensor (f.logsigma among them), the decisions audited; vs the reference's
    fp32 run at 2e-5 (value; the fixture holds the normalize=False runs).  normalize: every term over its own batch
    size (loss_scale 1 / B_u, 1 / N_s in the epilogue's gradients, the plane's rows included)."""
    from gpi import _lib as L
    from homosc_ref import oracle_homosc_fixture_elbo
    from elbo_ref import tensor_rel
    from gpu_masks import engine_relu_masks
    d = load('elbo_homosc_c32.npz')
    log_field = tag == 'log'
    model, bs = homosc_model(d, log_field)
    eps = (torch.cat([cuda(d['eps_enc']), cuda(d['eps_qz'])]), cuda(d['eps_qX']))
    elbo = model.elbo(step=0, armortized_bs=bs, eps=eps, normalize=normalize)
    (-elbo).backward()
    torch.cuda.synchronize()
    engine = model._elbo_engine(bs, int(d['cfg'][5]), normalize)
    last = engine.dec_descs[len(engine.dec_descs) - 1]
    assert engine.homosc and not engine.binary and last.cout == 1
    assert last.epilogue == (L.EPI_GAUSS_HOMO_LOSS if log_field else L.EPI_GAUSS_HOMO_EXP_LOSS)
    assert engine.dctx.ls_off == engine.flat.offset(model.f.logsigma) and engine.dctx.gls_off == engine.dec_gls_off >= 0
    assert engine.dctx.loss_scale[0] == (np.float32(1.0 / bs) if normalize else 1.0)
    terms = {}
    val_o, gr_o = oracle_homosc_fixture_elbo(d, masks=engine_relu_masks(engine), terms=terms, normalize=normalize,
                                             log_field=log_field)
    check_mask_audit()
    errs = {k: tensor_rel(p.grad.cpu().numpy(), gr_o[k]) for k, p in model.named_parameters()}
    print('homoscedastic %s elbo %.6f oracle %.6f reference %.6f, field logL oracle %r, worst gradient tensor %.2e, '
          'f.logsigma %.2e' % (tag, elbo.item(), val_o, float(d[tag + '.elbo']), (terms['logl_u'], terms['logl_s']),
                               max(errs.values()), errs['f.logsigma']))
    assert abs(elbo.item() - val_o) <= 1e-5 * abs(val_o), (elbo.item(), val_o)
    bad = {k: e for k, e in errs.items() if not e <= 5e-5}
    assert not bad, bad
    if not normalize:
        ref = float(d[tag + '.elbo'])
        assert abs(elbo.item() - ref) <= 2e-5 * abs(ref), (elbo.item(), ref)


def _step(d, model, bs, **kw):
    from gpi.train import FusedElboStep
    kw.setdefault('lr', 1e-3)
    kw.setdefault('seed', 7)
    return FusedElboStep(model, cuda(d['Xu']), bs, cuda(d['Xs']), cuda(d['Y']), cuda(d['F']), **kw)


@pytest.mark.parametrize('tag', ['log', 'exp'])
def test_homosc_fused_step_matches_module_path(device, tag):
    """forward_backward() of FusedElboStep on a homoscedastic model against model.elbo + backward on the step's own
    subset and noise (as test_gpu_binary_elbo's): ELBO 1e-5 relative, every gradient tensor within 1e-4 of its max."""
    d = load('elbo_homosc_c32.npz')
    model, bs = homosc_model(d, tag == 'log')
    ref_model, _ = homosc_model(d, tag == 'log')
    step = _step(d, model, bs)
    e = step.engine
    assert e.homosc and e.dec_gls_off >= 0
    for it in range(2):
        with torch.no_grad():
            for (k, p), (k2, q) in zip(model.named_parameters(), ref_model.named_parameters()):
                assert k == k2
                q.copy_(p)
        eps = (e.eps_z().clone(), e.eps_x().clone())
        ref_model._datasets['unsupervised'].perm = step.idx.clone().long()
        ref_model.zero_grad()
        ref = ref_model.elbo(step=it, armortized_bs=bs, eps=eps)
        (-ref).backward()
        step.forward_backward()
        torch.cuda.synchronize()
        got = step.elbo().item()
        assert abs(got - ref.item()) <= 1e-5 * abs(ref.item()), (it, got, ref.item())
        G = step.flat.G
        for k, p in ref_model.named_parameters():
            g = G[step.flat.name_offsets[k]:step.flat.name_offsets[k] + p.numel()].view(p.shape)
            ref_g = p.grad if p.grad is not None else torch.zeros_like(p)
            err = (g - ref_g).abs().max().item() / max(ref_g.abs().max().item(), 1.0)
            assert err < 1e-4, (it, k, err)
        assert ref_model.f.logsigma.grad.abs().max().item() > 0
        step.update()
    torch.cuda.synchronize()
    step.check_handoff()
    step.engine.check_flag()


def test_homosc_captured_step_replays_eager_bitwise(device):
    """A captured homoscedastic step against an eager twin over 3 steps: parameters and ELBO bit for bit, and the
    plane has moved: Adam's first steps are lr sign(g) each, so a pixel whose gradient keeps its sign has moved by
    3 lr = 3e-3 (the median pixel), none by more, and hardly any stands still."""
    d = load('elbo_homosc_c32.npz')
    model_a, bs = homosc_model(d)
    model_b, _ = homosc_model(d)
    eager = _step(d, model_a, bs, seed=3)
    graph = _step(d, model_b, bs, seed=3)
    graph.capture()
    torch.cuda.synchronize()
    for n in range(3):
        eager.step()
        graph.step()
        torch.cuda.synchronize()
        assert graph.elbo().item() == eager.elbo().item(), (n, graph.elbo().item(), eager.elbo().item())
        assert torch.equal(graph.flat.P, eager.flat.P), n
    assert graph.graph is not None and graph.step_ctr.item() == eager.step_ctr.item() == 3
    moved = (model_b.f.logsigma.detach().cpu() - torch.tensor(d['state.f.logsigma'])).abs()
    assert 2.5e-3 < moved.median().item() and moved.max().item() < 3.1e-3, (moved.median().item(), moved.max().item())
    assert (moved > 0).float().mean().item() > 0.99
    graph.check_handoff()
    eager.check_handoff()


def test_homosc_plane_follows_adam_on_the_oracle_gradients(device):
    """Three steps of FusedElboStep (forward_backward + update, lr 1e-3): f.logsigma has moved and equals torch
    Adam applied to the fp64 oracle's f.logsigma gradients -- the oracle evaluated at each step's own parameters,
    subset and noise -- at the project's Adam tolerances (rtol 1e-5, atol 1e-6).  The oracle takes its own ReLU
    decisions here: the step's epilogue has cleared the BN statistics the kernels' decisions are read back with,
    and the plane's gradient reaches the loss without passing backward through a ReLU (elbo_ref.MASK_FREE's
    argument: a decision that differs at a near-zero activation leaves the forward values alone)."""
    from homosc_ref import oracle_homosc_elbo
    d = load('elbo_homosc_c32.npz')
    n, nc, dz, Nu, bs_, Ns = [int(v) for v in d['cfg']]
    model, bs = homosc_model(d)
    step = _step(d, model, bs)
    e = step.engine
    plane0 = torch.tensor(d['state.f.logsigma'])
    p_ref = plane0.clone().requires_grad_(True)
    opt = torch.optim.Adam([p_ref], lr=1e-3)
    for it in range(3):
        st = {k: torch.tensor(p.detach().cpu().numpy(), dtype=torch.float64, requires_grad=True)
              for k, p in model.named_parameters()}
        idx = step.idx.clone().long().cpu().numpy()
        ez, ex = e.eps_z().clone().cpu().numpy(), e.eps_x().clone().cpu().numpy()
        step.forward_backward()
        torch.cuda.synchronize()
        val = oracle_homosc_elbo(st, d['Xu'][idx], d['Xs'], d['Y'], d['F'], ez[:bs], ez[bs:], ex, nc, n // nc)
        (-val).backward()
        assert abs(step.elbo().item() - val.item()) <= 1e-5 * abs(val.item()), (it, step.elbo().item(), val.item())
        p_ref.grad = st['f.logsigma'].grad.float()
        opt.step()
        step.update()
    torch.cuda.synchronize()
    got = model.f.logsigma.detach().cpu()
    print('plane after 3 steps: max |moved| %.3e, max |got - torch Adam| %.3e' % (
        (got - plane0).abs().max().item(), (got - p_ref.detach()).abs().max().item()))
    assert (got - plane0).abs().median().item() > 2.5e-3
    torch.testing.assert_close(got, p_ref.detach(), rtol=1e-5, atol=1e-6)
    step.check_handoff()


def test_homosc_elbo_c64_small_batch_with_dropout(device):
    """The `highres` codec (64^2, blocks [1, 2, 1], ROM 8 x 8) with homoscedastic=True and droprate 0.2, B_u = 8 of
    a pool of 16, N_s = 4, random-init parameters, a seeded plane and synthetic fields: model.elbo + backward
    against the fp64 oracle with the kernels' ReLU decisions and the Dropout2d scales the call drew, 1e-5 (value)
    and 5e-5 per gradient tensor."""
    from factories.model import ModelFactory
    from homosc_ref import oracle_homosc_elbo
    from elbo_ref import tensor_rel
    from gpu_masks import engine_relu_masks
    from oracle import codec as ocodec
    from test_gpu_c64 import _DS as DS64
    n, Nu, bs, Ns = 64, 16, 8, 4
    torch.manual_seed(13)
    fac = ModelFactory.FromIdentifier('highres', homoscedastic=True)
    fac.set('device', 'cuda')
    fac.set('droprate', 0.2)
    physics_, model, _, encoder, _, _ = fac.setup()
    model.encoder = encoder.cuda()
    nc = physics_['rom'].grid.n
    assert physics_['fom'].grid.n == n and model.f._homoscedastic and tuple(model.f.logsigma.shape) == (n, n)
    rng = np.random.default_rng(164)
    with torch.no_grad():
        model.f.logsigma.copy_(torch.tensor(rng.normal(-1.0, 0.3, (n, n)), dtype=torch.float32))
    Xu = rng.normal(0.3, 0.6, (Nu, n, n)).astype(np.float32)
    Xs = rng.normal(0.3, 0.6, (Ns, n, n)).astype(np.float32)
    Y = rng.normal(0.0, 0.3, (Ns, (n + 1) * (n - 1))).astype(np.float32)
    F = np.zeros((Ns, (nc + 1) ** 2), dtype=np.float32)
    bnodes = [e for e in range((nc + 1) ** 2) if e % (nc + 1) in (0, nc)]
    F[:, bnodes] = rng.uniform(-0.5, 0.5, (Ns, len(bnodes)))
    model.register_datasets({'supervised': DS64(X=cuda(Xs), Y=cuda(Y), F_ROM_BC=cuda(F)),
                             'unsupervised': DS64(perm=torch.arange(Nu, device='cuda'), X=cuda(Xu))}, None,
                            create_unsupervised_variational_approximation=False)
    model.cuda()
    dz, dx = model.dim_latent, model.g.dim_effective_property
    eps_z = rng.normal(size=(bs + Ns, dz)).astype(np.float32)
    eps_x = rng.normal(size=(Ns, dx)).astype(np.float32)
    elbo = model.elbo(step=0, armortized_bs=bs, eps=(cuda(eps_z), cuda(eps_x)))
    (-elbo).backward()
    torch.cuda.synchronize()
    engine = model._elbo_engine(bs, Ns, False)
    assert engine.homosc and engine.has_dropout
    drops = {k: {nm: v.double().cpu() for nm, v in dd.items()} for k, dd in engine.dropout_views().items()}
    assert set(drops) == {'enc', 'dec'}
    masks = engine_relu_masks(engine)
    st = {k: torch.tensor(p.detach().cpu().numpy(), dtype=torch.float64, requires_grad=True)
          for k, p in model.named_parameters()}
    ocodec.MASK_AUDIT.clear()
    val = oracle_homosc_elbo(st, Xu[:bs], Xs, Y, F, eps_z[:bs], eps_z[bs:], eps_x, nc, n // nc, masks=masks,
                             drops=drops)
    check_mask_audit()
    (-val).backward()
    errs = {k: tensor_rel(p.grad.cpu().numpy(), st[k].grad.numpy()) for k, p in model.named_parameters()}
    print('homoscedastic c64 elbo %.6f oracle %.6f worst gradient tensor %.2e, f.logsigma %.2e' % (
        elbo.item(), val.item(), max(errs.values()), errs['f.logsigma']))
    assert abs(elbo.item() - val.item()) <= 1e-5 * abs(val.item()), (elbo.item(), val.item())
    bad = {k: e for k, e in errs.items() if not e <= 5e-5}
    assert not bad, bad


def _force_homosc_decoder(monkeypatch):
    """The fixture model builders of the other test modules construct CNNDecoder(...): make them build the
    homoscedastic decoder."""
    import bottleneck.Decoder as D
    real = D.HomoscedasticCNNDecoder

    def homosc(*a, **k):
        assert a[6] is False
        return real(*a, **k)

    monkeypatch.setattr(D, 'CNNDecoder', homosc)


@pytest.mark.parametrize('holdoff', [False, True], ids=['active', 'holdoff'])
def test_homosc_elbo_with_vo_term(device, monkeypatch, holdoff):
    """The VO term with a homoscedastic decoder (third decoder group through the epilogue with its own loss_scale):
    vo_elbo_c32.npz's model, VO queries and noise with a seeded plane (homosc_ref.homosc_vo_fixture; N_vo = 4,
    freeX), two VO updates, then model.elbo + backward, the term active or held off, against the fp64 oracle with
    the kernels' ReLU decisions of all four codec calls: 1e-5 (value), 5e-5 per gradient tensor."""
    from homosc_ref import homosc_vo_fixture, oracle_homosc_vo_fixture_elbo
    from elbo_ref import tensor_rel
    from gpu_masks import engine_relu_masks
    from oracle import codec as ocodec
    import test_gpu_vo as tv
    _force_homosc_decoder(monkeypatch)
    d = homosc_vo_fixture(tv.load('vo_elbo_c32.npz'))
    model, ens, bs = tv.build_vo_model(d, independent_X=True)
    assert model.f._homoscedastic
    np.testing.assert_array_equal(model.f.logsigma.detach().cpu().numpy(), d['state.f.logsigma'])
    Ns, Nvo = int(d['cfg'][5]), int(d['cfg'][6])
    assert Nvo == 4
    for it in range(2):
        model.update_virtual_observables(int(d['cfg'][7]), step=it,
                                         eps=(cuda(d['upd%d.eps_X' % it]), cuda(d['upd%d.eps_y' % it])))
    ens.check_flag()
    vo_mean, vo_vars = ens.mean.cpu().numpy(), ens.vars.cpu().numpy()
    if holdoff:
        h = [cuda(d['epsh%d' % i]) for i in range(4)]
        eps = (torch.cat([h[0], h[1], h[3]]), h[2])
    else:
        e = [cuda(d['eps%d' % i]) for i in range(6)]
        eps = (torch.cat([e[0], e[1], e[3]]), torch.cat([e[2], e[4]]), e[5])
    elbo = model.elbo(step=0, armortized_bs=bs, vo_holdoff=holdoff, eps=eps)
    (-elbo).backward()
    torch.cuda.synchronize()
    engine = model._elbo_engine(bs, Ns, False, N_vo=Nvo, vo_holdoff=holdoff)
    assert engine.homosc and engine.g_vo == 2 and engine.B == bs + Ns + Nvo
    masks = engine_relu_masks(engine)
    assert set(masks) == {'enc', 'dec_u', 'dec_s', 'dec_v'}
    ocodec.MASK_AUDIT.clear()
    terms = {}
    val_o, gr_o = oracle_homosc_vo_fixture_elbo(d, vo_mean, vo_vars, masks=masks, holdoff=holdoff, terms=terms)
    check_mask_audit()
    errs = {k: tensor_rel(p.grad.cpu().numpy(), gr_o[k]) for k, p in model.named_parameters() if k in gr_o}
    print('homoscedastic vo elbo %.6f oracle %.6f field logL %r worst gradient tensor %.2e, f.logsigma %.2e' % (
        elbo.item(), val_o, (terms['logl_u'], terms['logl_s'], terms['logl_v']), max(errs.values()),
        errs['f.logsigma']))
    assert abs(elbo.item() - val_o) <= 1e-5 * abs(val_o), (elbo.item(), val_o)
    bad = {k: v for k, v in errs.items() if not v <= 5e-5}
    assert not bad, bad
    for k, p in model.named_parameters():            # what the oracle's objective does not reach (held-off q_X['vo'])
        if k not in gr_o:
            assert p.grad is None or not p.grad.any(), k


def test_homosc_prediction_ensemble_update(device, monkeypatch):
    """One PredictionEnsemble.update (PredictionEnsembleEngine: the hold-off ELBO engine with B_u = N_s = 0, the
    homoscedastic epilogue on its one decoder group reading the shadow decoder's plane, Adam on the q_z rows)
    against a torch fp64 restatement of its objective -- logL_x(decoder(mean + exp(logsigma) eps)) - KL(q_z), one
    Adam step at lr 1e-2 -- at 1e-4: the three logged values, the q_z gradient and q_z after the step.  The shadow
    holds the model's plane, no per-sample rows exist (gls_off = -1) and the plane's gradient region stays zero."""
    from homosc_ref import homosc_decoder
    from elbo_ref import CODEC
    from oracle import elbo as oelbo
    from oracle import codec as ocodec
    from gpu_masks import engine_relu_masks
    from bottleneck.components import PredictionEnsemble
    from lamp.optimization import LearningScheduleWrapper
    import test_gpu_predictive as tp
    _force_homosc_decoder(monkeypatch)
    d = dict(tp.load('pe_analysis_c32.npz'))
    k3 = 'state.f.features.LastTransUp.conv3.weight'
    d[k3] = np.ascontiguousarray(d[k3][:1])
    n, nc, dz, Nval = [int(v) for v in d['cfg'][:4]]
    rng = np.random.default_rng(15)
    d['state.f.logsigma'] = rng.normal(-1.0, 0.3, (n, n)).astype(np.float32)
    model, ds = tp.build(d)
    assert model.f._homoscedastic
    np.testing.assert_array_equal(model.f.logsigma.detach().cpu().numpy(), d['state.f.logsigma'])
    pe = PredictionEnsemble(model, ds, LearningScheduleWrapper.Dummy(), lr=1e-2, writer=tp._Writer())
    m0 = rng.normal(0, 0.5, (Nval, dz)).astype(np.float32)
    l0 = rng.normal(-1.0, 0.3, (Nval, dz)).astype(np.float32)
    eps = rng.normal(size=(Nval, dz)).astype(np.float32)
    pe.q_z.init(cuda(m0), cuda(l0))
    pe.update(numIter=1, record=True, step=0, eps=[cuda(eps)])
    torch.cuda.synchronize()
    eng = pe._engine
    ee = eng.engine
    assert ee.homosc and ee.B_u == 0 and ee.N_s == 0 and ee.vo_holdoff and not ee.shared_grads
    assert ee.dec_gls_off == -1 and ee.dctx.gls_off == -1 and ee.dctx.ls_off == eng.flat.offset(eng.shadow.logsigma)
    np.testing.assert_array_equal(eng.shadow.logsigma.detach().cpu().numpy(), d['state.f.logsigma'])
    o = eng.flat.offset(eng.shadow.logsigma)
    assert not eng.flat.gacc[o:o + n * n].any() and not eng.flat.G[o:o + n * n].any()
    # ---- fp64 restatement
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
    mean, ls = t(m0).requires_grad_(True), t(l0).requires_grad_(True)
    dec_p = {k[8:]: t(v) for k, v in d.items() if k.startswith('state.f.') and v.dtype.kind == 'f'
             and not k.endswith(('running_mean', 'running_var'))}
    masks = engine_relu_masks(ee)
    assert set(masks) == {'dec_v'}
    ocodec.MASK_AUDIT.clear()
    mx, lsx = homosc_decoder(dec_p, CODEC[n], masks['dec_v'])(oelbo.reparam(mean, ls, t(eps)))
    check_mask_audit(max_frac=1e-4)
    logL = oelbo.dgll(t(d['X']), mx, 2 * lsx)
    KLD = oelbo.kl_unit(mean, 2 * ls)
    elbo = logL - KLD
    opt = torch.optim.Adam([mean, ls], lr=1e-2)
    (-elbo).backward()
    g_mean, g_ls = mean.grad.clone(), ls.grad.clone()
    opt.step()
    w = pe.writer.d
    print('homoscedastic PE values', {k: (w['PredictionEnsemble/' + k], r.item()) for k, r in (('logL', logL), ('KLD', KLD))})
    for k, ref in (('elbo', elbo), ('logL', logL), ('KLD', KLD)):
        assert abs(w['PredictionEnsemble/' + k] - ref.item()) <= 1e-4 * abs(ref.item()), (k, w, ref.item())
    G, fl = eng.flat.G, eng.flat
    for q, g in ((pe.q_z._mean, g_mean), (pe.q_z._logsigma, g_ls)):
        o = fl.offset(q)
        assert tp.rel(G[o:o + q.numel()].view(q.shape).cpu(), g) < 1e-4
    assert tp.rel(pe.q_z.mean.detach().cpu(), mean.detach()) < 1e-4
    assert tp.rel(pe.q_z.logsigma.detach().cpu(), ls.detach()) < 1e-4
    assert tp.rel(pe.q_z.mean.detach().cpu(), m0) > 1e-3, 'the step moved q_z'


def test_homosc_decoder_forward_train_eval_and_samples(device):
    """HomoscedasticCNNDecoder.forward in training mode (DecoderEngine with a plain-store one-channel output
    conv; backward through it, the plane's gradient through the expanded view) and in eval mode (EvalDecoderEngine),
    with and without flatten, and propagate_samples: shapes as the reference's, the log-sigma output the plane
    itself, the mean at 1e-5 of the fp64 codec (training: with the kernels' ReLU decisions; every parameter
    gradient and the latent's at 5e-5 per tensor; eval: tests/eval_ref.py)."""
    from homosc_ref import homosc_decoder
    from eval_ref import decoder_eval
    from elbo_ref import CODEC, tensor_rel
    from gpu_masks import codec_engine_masks
    from oracle import codec as ocodec
    d = load('elbo_homosc_c32.npz')
    model, _ = homosc_model(d)
    dec = model.f
    assert dec.training
    rng = np.random.default_rng(121)
    B = 5
    z = rng.normal(size=(B, dec.dim_latent)).astype(np.float32)
    R = rng.normal(size=(B, 32, 32)).astype(np.float32)
    R2 = rng.normal(size=(B, 32, 32)).astype(np.float32)
    Z = cuda(z).requires_grad_(True)
    mean, lsig = dec(Z)
    assert tuple(mean.shape) == tuple(lsig.shape) == (B, 32, 32)
    assert torch.equal(lsig.detach(), dec.logsigma.detach().expand(B, 32, 32))
    fm, fl = dec(Z, flatten=True)
    assert tuple(fm.shape) == tuple(fl.shape) == (B, 32 * 32)
    assert torch.equal(fm.detach().view(B, 32, 32), mean.detach()) and torch.equal(fl.detach().view(B, 32, 32), lsig.detach())
    samples = dec.propagate_samples(Z)
    assert tuple(samples.shape) == (B, 32, 32) and bool(torch.isfinite(samples).all())
    dec.zero_grad()
    Z.grad = None
    mean, lsig = dec(Z)
    e = next(iter(dec._gpi_engines.values()))
    masks = codec_engine_masks(e, B)
    ((mean * cuda(R)).sum() + (lsig * cuda(R2)).sum()).backward()
    torch.cuda.synchronize()
    pd = {k: torch.tensor(p.detach().cpu().numpy(), dtype=torch.float64, requires_grad=True)
          for k, p in dec.named_parameters()}
    Zo = torch.tensor(z, dtype=torch.float64, requires_grad=True)
    ocodec.MASK_AUDIT.clear()
    mean_o, lsig_o = homosc_decoder(pd, CODEC[32], masks)(Zo)
    check_mask_audit(max_frac=1e-4)
    ((mean_o * torch.tensor(R, dtype=torch.float64)).sum() + (lsig_o * torch.tensor(R2, dtype=torch.float64)).sum()).backward()
    assert tensor_rel(mean.detach().cpu().numpy(), mean_o.detach().numpy()) <= 1e-5
    errs = {k: tensor_rel(p.grad.cpu().numpy(), pd[k].grad.numpy()) for k, p in dec.named_parameters()}
    errs['Z'] = tensor_rel(Z.grad.cpu().numpy(), Zo.grad.numpy())
    bad = {k: v for k, v in errs.items() if not v <= 5e-5}
    assert not bad, bad
    # ---- eval mode
    gen = torch.Generator().manual_seed(11)
    with torch.no_grad():
        for m in dec.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.copy_(0.5 * torch.randn(m.running_mean.shape, generator=gen))
                m.running_var.copy_(0.5 + torch.rand(m.running_var.shape, generator=gen))
    dec.eval()
    with torch.no_grad():
        mean_e, lsig_e = dec(cuda(z))
        fm, fl = dec(cuda(z), flatten=True)
        samples = dec.propagate_samples(cuda(z))
    assert tuple(mean_e.shape) == tuple(lsig_e.shape) == tuple(samples.shape) == (B, 32, 32)
    assert tuple(fm.shape) == tuple(fl.shape) == (B, 32 * 32) and torch.equal(fm.view(B, 32, 32), mean_e)
    assert torch.equal(lsig_e, dec.logsigma.detach().expand(B, 32, 32))
    p64 = {k: v.detach().cpu().double() for k, v in dec.state_dict().items()
           if v.dtype.is_floating_point and k != 'logsigma'}
    w = p64['features.LastTransUp.conv3.weight']
    p64['features.LastTransUp.conv3.weight'] = torch.cat([w, torch.zeros_like(w)], 0)   # (the helper reads 2 channels)
    ref = decoder_eval(p64, torch.tensor(z, dtype=torch.float64), 8, [1, 1], 4, 4)[0].numpy()
    got = mean_e.cpu().numpy()
    assert tensor_rel(got, ref) <= 1e-5, tensor_rel(got, ref)
    assert np.ptp(got) > 100 * 1e-5 * np.abs(ref).max(), 'the image varies by far more than the bar'


def _shape_info():
    from gpi import _lib as L
    info = (C.c_int64 * 4)()
    assert L.lib().gpi_conv_shape_info(info) == 0
    return list(info)


def test_default_decoder_plans_the_launches_it_did(device):
    """Guard of the default (two-channel) path: one eager step of the bench workload plans its 45 conv launches
    (23 encoder + decoder forwards, 22 backwards incl. the fused output conv), every one on its compile-time
    shape, as tests/test_gpu_shapes.py states for it; the same workload with homoscedastic=True plans 45 too, all
    on their shapes but the fused output conv (no csrc/conv_shapes.h entry: the generic kernel)."""
    import bench
    from factories.model import ModelFactory
    from gpi.train import FusedElboStep

    def planned_matched(model, data, B_u):
        Xu, Xs, Y, F = data
        step = FusedElboStep(model, Xu, B_u, Xs, Y, F, lr=1e-2, seed=4321, subset_seed=777)
        step.step_eager()
        torch.cuda.synchronize()
        n0 = _shape_info()
        step.step_eager()
        torch.cuda.synchronize()
        n1 = _shape_info()
        return n1[1] - n0[1], n1[2] - n0[2], step

    model, data, (B_u, N_s), _ = bench.build('c64', device, seed=1)
    planned, matched, step = planned_matched(model, data, B_u)
    assert not step.engine.homosc and step.engine.dctx.ls_off == -1 and step.engine.dctx.gls_off == -1
    assert (planned, matched) == (45, 45), (planned, matched)
    del step, model
    real = ModelFactory.FromIdentifier
    ModelFactory.FromIdentifier = classmethod(lambda cls, ident, *a, **k: real(ident, *a, homoscedastic=True, **k))
    try:
        model, data, (B_u, N_s), _ = bench.build('c64', device, seed=1)
    finally:
        ModelFactory.FromIdentifier = real
    planned, matched, step = planned_matched(model, data, B_u)
    assert step.engine.homosc and bool(torch.isfinite(step.elbo()).item())
    assert (planned, matched) == (45, 44), (planned, matched)
