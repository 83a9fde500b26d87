"""The ELBO with the binary (two-phase) decoder on the GPU: GenerativeModel.elbo + backward, the fused training
step (eager and captured), the C64 codec with dropout, the VO term (active / held off), one PredictionEnsemble
update and the training- and eval-mode forward of a binary CNNDecoder, against the fp64 oracle
(tests/binary_ref.py, with the kernels' ReLU decisions) and the reference run of
tests/golden/elbo_binary_c32.npz.  Every logit of the fixture stays below 15 in magnitude (asserted where the
fixture is made and in tests/test_binary_oracle.py)."""
import numpy as np
import pytest
import torch

from test_gpu_parity import load, cuda, _DS
from test_gpu_c64 import check_mask_audit

pytestmark = pytest.mark.gpu


def binary_model(d):
    """The fixture's model on the GPU: test_gpu_parity.build_golden_model with the binary decoder."""
    from bottleneck.Encoder import CNNEncoder
    from bottleneck.Decoder import CNNDecoder
    from bottleneck.components import EffectivePropertyMap, ReducedOrderModelOperator
    from bottleneck.ROM import ROM
    from bottleneck.generative import GenerativeModel
    from physics.grid import StructuredGrid
    n, nc, dz, Nu, bs, Ns = [int(v) for v in d['cfg']]
    enc = CNNEncoder(n, dz, [1, 1], 4, 4, drop_rate=0)
    dec = CNNDecoder(n, dz, (8, 8), 1, 4, [1, 1], True, 4, drop_rate=0.)
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
    return model, bs


@pytest.mark.parametrize('normalize', [False, True], ids=['sum', 'normalize'])
def test_binary_elbo_module_path_c32(device, normalize):
    """model.elbo + backward on the fixture's inputs and noise: vs the fp64 oracle with the kernels' ReLU
    decisions at 1e-5 (value) and 5e-5 per gradient tensor, the decisions audited; vs the reference's fp32 run
    at 2e-5 (value; the fixture holds the normalize=False run).  normalize: every term over its own batch size
    (loss_scale 1 / B_u, 1 / N_s in the epilogue's gradient)."""
    from binary_ref import oracle_binary_fixture_elbo
    from elbo_ref import tensor_rel
    from gpu_masks import engine_relu_masks
    d = load('elbo_binary_c32.npz')
    model, bs = binary_model(d)
    eps = (torch.cat([cuda(d['eps_enc']), cuda(d['eps_qz'])]), cuda(d['eps_qX']))
    elbo = model.elbo(step=0, armortized_bs=bs, eps=eps, normalize=normalize)
    (-elbo).backward()
    torch.cuda.synchronize()
    engine = model._elbo_engine(bs, int(d['cfg'][5]), normalize)
    assert engine.binary and engine.dec_descs[len(engine.dec_descs) - 1].cout == 1
    assert engine.dctx.loss_scale[0] == (np.float32(1.0 / bs) if normalize else 1.0)
    terms = {}
    val_o, gr_o = oracle_binary_fixture_elbo(d, masks=engine_relu_masks(engine), terms=terms, normalize=normalize)
    check_mask_audit()
    errs = {k: tensor_rel(p.grad.cpu().numpy(), gr_o[k]) for k, p in model.named_parameters()}
    print('binary elbo %.6f oracle %.6f reference %.6f, field logL oracle %r, worst gradient tensor %.2e' % (
        elbo.item(), val_o, float(d['elbo']), (terms['logl_u'], terms['logl_s']), max(errs.values())))
    assert abs(elbo.item() - val_o) <= 1e-5 * abs(val_o), (elbo.item(), val_o)
    bad = {k: e for k, e in errs.items() if not e <= 5e-5}
    assert not bad, bad
    if not normalize:
        assert abs(elbo.item() - float(d['elbo'])) <= 2e-5 * abs(float(d['elbo'])), (elbo.item(), float(d['elbo']))


def _step(d, model, bs, **kw):
    from gpi.train import FusedElboStep
    kw.setdefault('lr', 1e-3)
    kw.setdefault('seed', 7)
    return FusedElboStep(model, cuda(d['Xu']), bs, cuda(d['Xs']), cuda(d['Y']), cuda(d['F']), **kw)


def test_binary_fused_step_matches_module_path(device):
    """One forward_backward() of FusedElboStep on a binary model against model.elbo + backward on the step's own
    subset and noise (as test_gpu_fused_vo.one_round): ELBO 1e-5 relative, every gradient tensor within 1e-4 of
    its max.  The step binds the pool: its low-phase value is the pool's minimum, the batch's too here (every
    image holds both phases)."""
    d = load('elbo_binary_c32.npz')
    model, bs = binary_model(d)
    ref_model, _ = binary_model(d)
    step = _step(d, model, bs)
    e = step.engine
    assert e.binary and e.dctx.tgt_lo[0] == float(d['Xu'].min()) == e.dctx.tgt_lo[1]
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
        step.update()
    torch.cuda.synchronize()
    step.check_handoff()
    step.engine.check_flag()


def test_binary_captured_step_replays_eager_bitwise(device):
    """A captured binary step against an eager twin over 3 steps: parameters and ELBO bit for bit."""
    d = load('elbo_binary_c32.npz')
    model_a, bs = binary_model(d)
    model_b, _ = binary_model(d)
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
    graph.check_handoff()
    eager.check_handoff()


def test_binary_eval_decoder_returns_probabilities(device):
    """EvalDecoderEngine (CNNDecoder.eval() forward) of a binary decoder: the probability image against the fp64
    eval-mode restatement (tests/eval_ref.py) followed by the sigmoid, 1e-5 of the image's max."""
    from eval_ref import decoder_eval
    from elbo_ref import tensor_rel
    d = load('elbo_binary_c32.npz')
    model, _ = binary_model(d)
    dec = model.f
    gen = torch.Generator().manual_seed(11)
    with torch.no_grad():
        for m in dec.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.copy_(0.5 * torch.randn(m.running_mean.shape, generator=gen))
                m.running_var.copy_(0.5 + torch.rand(m.running_var.shape, generator=gen))
    dec.eval()
    z = torch.randn(3, dec.dim_latent, generator=gen)
    with torch.no_grad():
        prob = dec(z.cuda())
    assert tuple(prob.shape) == (3, 32, 32)
    p64 = {k: v.detach().cpu().double() for k, v in dec.state_dict().items() if v.dtype.is_floating_point}
    w = p64['features.LastTransUp.conv3.weight']
    p64['features.LastTransUp.conv3.weight'] = torch.cat([w, torch.zeros_like(w)], 0)   # (the helper reads 2 channels)
    logit = decoder_eval(p64, z.double(), 8, [1, 1], 4, 4)[0]
    assert float(logit.abs().max()) < 15
    ref = torch.sigmoid(logit).numpy()
    got = prob.cpu().numpy()
    assert got.min() >= 0.0 and got.max() <= 1.0
    assert tensor_rel(got, ref) <= 1e-5, tensor_rel(got, ref)
    assert np.ptp(got) > 100 * 1e-5 * np.abs(ref).max(), 'the image varies by far more than the bar'


def test_binary_elbo_c64_small_batch_with_dropout(device):
    """The `highres` codec (64^2, blocks [1, 2, 1], ROM 8 x 8) with binary_field=True and droprate 0.2, B_u = 8 of
    a pool of 16, N_s = 4, random-init parameters and two-valued synthetic fields: model.elbo + backward against
    the fp64 oracle with the kernels' ReLU decisions and the Dropout2d scales the call drew, 1e-5 (value) and 5e-5
    per gradient tensor."""
    from factories.model import ModelFactory
    from binary_ref import oracle_binary_elbo, two_phase, LOGIT_MAX
    from elbo_ref import tensor_rel
    from gpu_masks import engine_relu_masks
    from oracle import codec as ocodec
    from test_gpu_c64 import _DS as DS64
    n, Nu, bs, Ns = 64, 16, 8, 4
    torch.manual_seed(13)
    fac = ModelFactory.FromIdentifier('highres', binary_field=True)
    fac.set('device', 'cuda')
    fac.set('droprate', 0.2)
    physics_, model, _, encoder, _, _ = fac.setup()
    model.encoder = encoder.cuda()
    nc = physics_['rom'].grid.n
    assert physics_['fom'].grid.n == n and model.f._binary
    rng = np.random.default_rng(64)
    Xu = two_phase(rng.normal(0.3, 0.6, (Nu, n, n)))
    Xs = two_phase(rng.normal(0.3, 0.6, (Ns, n, n)))
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
    assert engine.binary and engine.has_dropout
    drops = {k: {nm: v.double().cpu() for nm, v in dd.items()} for k, dd in engine.dropout_views().items()}
    assert set(drops) == {'enc', 'dec'}
    masks = engine_relu_masks(engine)
    st = {k: torch.tensor(p.detach().cpu().numpy(), dtype=torch.float64, requires_grad=True)
          for k, p in model.named_parameters()}
    ocodec.MASK_AUDIT.clear()
    terms = {}
    val = oracle_binary_elbo(st, Xu[:bs], Xs, Y, F, eps_z[:bs], eps_z[bs:], eps_x, nc, n // nc, masks=masks,
                             drops=drops, terms=terms)
    check_mask_audit()
    assert terms['logit_max'] < LOGIT_MAX
    (-val).backward()
    errs = {k: tensor_rel(p.grad.cpu().numpy(), st[k].grad.numpy()) for k, p in model.named_parameters()}
    print('binary c64 elbo %.6f oracle %.6f worst gradient tensor %.2e' % (elbo.item(), val.item(), max(errs.values())))
    assert abs(elbo.item() - val.item()) <= 1e-5 * abs(val.item()), (elbo.item(), val.item())
    bad = {k: e for k, e in errs.items() if not e <= 5e-5}
    assert not bad, bad


def _force_binary_decoder(monkeypatch):
    """The fixture model builders of the other test modules construct CNNDecoder(..., binary=False, ...)
    positionally: make them build the binary decoder."""
    import bottleneck.Decoder as D
    real = D.CNNDecoder

    def binary(*a, **k):
        a = list(a)
        assert a[6] is False
        a[6] = True
        return real(*a, **k)

    monkeypatch.setattr(D, 'CNNDecoder', binary)


@pytest.mark.parametrize('holdoff', [False, True], ids=['active', 'holdoff'])
def test_binary_elbo_with_vo_term(device, monkeypatch, holdoff):
    """The VO term with a binary decoder (third decoder group through the Bernoulli epilogue, its own tgt_lo):
    vo_elbo_c32.npz's model, VO queries and noise with two-valued decoder targets (binary_ref.binary_vo_fixture;
    N_vo = 4, freeX), two VO updates, then model.elbo + backward, the term active or held off, against the fp64
    oracle with the kernels' ReLU decisions of all four codec calls: 1e-5 (value), 5e-5 per gradient tensor."""
    from binary_ref import binary_vo_fixture, oracle_binary_vo_fixture_elbo, LOGIT_MAX
    from elbo_ref import tensor_rel
    from gpu_masks import engine_relu_masks
    from oracle import codec as ocodec
    import test_gpu_vo as tv
    _force_binary_decoder(monkeypatch)
    d = binary_vo_fixture(tv.load('vo_elbo_c32.npz'))
    model, ens, bs = tv.build_vo_model(d, independent_X=True)
    assert model.f._binary
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
    assert engine.binary and engine.g_vo == 2 and engine.dctx.tgt_lo[2] == float(d['Xv'].min())
    masks = engine_relu_masks(engine)
    assert set(masks) == {'enc', 'dec_u', 'dec_s', 'dec_v'}
    ocodec.MASK_AUDIT.clear()
    terms = {}
    val_o, gr_o = oracle_binary_vo_fixture_elbo(d, vo_mean, vo_vars, masks=masks, holdoff=holdoff, terms=terms)
    check_mask_audit()
    assert terms['logit_max'] < LOGIT_MAX
    errs = {k: tensor_rel(p.grad.cpu().numpy(), gr_o[k]) for k, p in model.named_parameters() if k in gr_o}
    print('binary vo elbo %.6f oracle %.6f field logL %r worst gradient tensor %.2e' % (
        elbo.item(), val_o, (terms['logl_u'], terms['logl_s'], terms['logl_v']), max(errs.values())))
    assert abs(elbo.item() - val_o) <= 1e-5 * abs(val_o), (elbo.item(), val_o)
    bad = {k: v for k, v in errs.items() if not v <= 5e-5}
    assert not bad, bad
    for k, p in model.named_parameters():            # what the oracle's objective does not reach (held-off q_X['vo'])
        if k not in gr_o:
            assert p.grad is None or not p.grad.any(), k


def test_binary_prediction_ensemble_update(device, monkeypatch):
    """One PredictionEnsemble.update (PredictionEnsembleEngine: the hold-off ELBO engine with B_u = N_s = 0, the
    Bernoulli epilogue on its one decoder group, Adam on the q_z rows) with a binary decoder against a torch fp64
    restatement of its objective -- logL_x(decoder(mean + exp(logsigma) eps)) - KL(q_z), one Adam step at lr 1e-2
    -- at 1e-4: the three logged values, the q_z gradient and q_z after the step."""
    from binary_ref import binary_decoder, bernoulli_loglik, two_phase, LOGIT_MAX
    from elbo_ref import CODEC
    from oracle import elbo as oelbo
    from oracle import codec as ocodec
    from gpu_masks import engine_relu_masks
    from bottleneck.components import PredictionEnsemble
    from lamp.optimization import LearningScheduleWrapper
    import test_gpu_predictive as tp
    _force_binary_decoder(monkeypatch)
    d = dict(tp.load('pe_analysis_c32.npz'))
    d['X'] = two_phase(d['X'])
    k3 = 'state.f.features.LastTransUp.conv3.weight'
    d[k3] = np.ascontiguousarray(d[k3][:1])
    model, ds = tp.build(d)
    assert model.f._binary
    n, nc, dz, Nval = [int(v) for v in d['cfg'][:4]]
    pe = PredictionEnsemble(model, ds, LearningScheduleWrapper.Dummy(), lr=1e-2, writer=tp._Writer())
    rng = np.random.default_rng(5)
    m0 = rng.normal(0, 0.5, (Nval, dz)).astype(np.float32)
    l0 = rng.normal(-1.0, 0.3, (Nval, dz)).astype(np.float32)
    eps = rng.normal(size=(Nval, dz)).astype(np.float32)
    pe.q_z.init(cuda(m0), cuda(l0))
    pe.update(numIter=1, record=True, step=0, eps=[cuda(eps)])
    torch.cuda.synchronize()
    eng = pe._engine
    assert eng.engine.binary and eng.engine.B_u == 0 and eng.engine.N_s == 0 and eng.engine.vo_holdoff
    assert eng.engine.dctx.tgt_lo[0] == float(d['X'].min())
    # ---- fp64 restatement
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
    mean, ls = t(m0).requires_grad_(True), t(l0).requires_grad_(True)
    dec_p = {k[8:]: t(v) for k, v in d.items() if k.startswith('state.f.') and v.dtype.kind == 'f'
             and not k.endswith(('running_mean', 'running_var'))}
    # (the kernels' ReLU decisions, as every oracle comparison here: a decision that differs at a near-zero
    # activation leaves the values alone and moves the gradient)
    masks = engine_relu_masks(eng.engine)
    assert set(masks) == {'dec_v'}
    ocodec.MASK_AUDIT.clear()
    a = binary_decoder(dec_p, CODEC[n], masks['dec_v'])(oelbo.reparam(mean, ls, t(eps)))
    check_mask_audit(max_frac=1e-4)
    assert float(a.detach().abs().max()) < LOGIT_MAX
    logL = bernoulli_loglik(t(d['X']), a)
    KLD = oelbo.kl_unit(mean, 2 * ls)
    elbo = logL - KLD
    opt = torch.optim.Adam([mean, ls], lr=1e-2)
    (-elbo).backward()
    g_mean, g_ls = mean.grad.clone(), ls.grad.clone()
    opt.step()
    w = pe.writer.d
    print('binary PE values', {k: (w['PredictionEnsemble/' + k], r.item()) for k, r in (('logL', logL), ('KLD', KLD))})
    for k, ref in (('elbo', elbo), ('logL', logL), ('KLD', KLD)):
        assert abs(w['PredictionEnsemble/' + k] - ref.item()) <= 1e-4 * abs(ref.item()), (k, w, ref.item())
    G, fl = eng.flat.G, eng.flat
    for q, g in ((pe.q_z._mean, g_mean), (pe.q_z._logsigma, g_ls)):
        o = fl.offset(q)
        assert tp.rel(G[o:o + q.numel()].view(q.shape).cpu(), g) < 1e-4
    assert tp.rel(pe.q_z.mean.detach().cpu(), mean.detach()) < 1e-4
    assert tp.rel(pe.q_z.logsigma.detach().cpu(), ls.detach()) < 1e-4
    assert tp.rel(pe.q_z.mean.detach().cpu(), m0) > 1e-3, 'the step moved q_z'


def test_binary_decoder_training_forward_backward(device):
    """CNNDecoder(binary=True).forward in training mode (DecoderEngine with a plain-store one-channel output conv,
    torch.sigmoid on its logit image, backward through the one-channel conv): the probability image against
    sigmoid of the fp64 codec with the kernels' ReLU decisions at 1e-5, every parameter gradient and the
    latent's at 5e-5 per tensor."""
    from binary_ref import binary_decoder
    from elbo_ref import CODEC, tensor_rel
    from gpu_masks import codec_engine_masks
    from oracle import codec as ocodec
    d = load('elbo_binary_c32.npz')
    model, _ = binary_model(d)
    dec = model.f
    assert dec.training
    rng = np.random.default_rng(21)
    B = 5
    z = rng.normal(size=(B, dec.dim_latent)).astype(np.float32)
    R = rng.normal(size=(B, 32, 32)).astype(np.float32)
    Z = cuda(z).requires_grad_(True)
    prob = dec(Z)
    assert not isinstance(prob, tuple) and tuple(prob.shape) == (B, 32, 32)
    flat = dec(Z, flatten=True)
    assert tuple(flat.shape) == (B, 32 * 32) and torch.equal(flat.detach().view(B, 32, 32), prob.detach())
    dec.zero_grad()
    Z.grad = None
    prob = dec(Z)
    e = next(iter(dec._gpi_engines.values()))
    masks = codec_engine_masks(e, B)
    (prob * cuda(R)).sum().backward()
    torch.cuda.synchronize()
    pd = {k: torch.tensor(p.detach().cpu().numpy(), dtype=torch.float64, requires_grad=True)
          for k, p in dec.named_parameters()}
    Zo = torch.tensor(z, dtype=torch.float64, requires_grad=True)
    ocodec.MASK_AUDIT.clear()
    logit = binary_decoder(pd, CODEC[32], masks)(Zo)
    check_mask_audit(max_frac=1e-4)
    assert float(logit.detach().abs().max()) < 15
    prob_o = torch.sigmoid(logit)
    (prob_o * torch.tensor(R, dtype=torch.float64)).sum().backward()
    assert tensor_rel(prob.detach().cpu().numpy(), prob_o.detach().numpy()) <= 1e-5
    errs = {k: tensor_rel(p.grad.cpu().numpy(), pd[k].grad.numpy()) for k, p in dec.named_parameters()}
    errs['Z'] = tensor_rel(Z.grad.cpu().numpy(), Zo.grad.numpy())
    bad = {k: v for k, v in errs.items() if not v <= 5e-5}
    assert not bad, bad
