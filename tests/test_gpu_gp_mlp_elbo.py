"""The ELBO with hidden layers in the effective-property map on the GPU: GenerativeModel.elbo + backward on the
three cases of tests/golden/elbo_gpmlp_c32.npz (free-X L = 1, 2; lock-X L = 1) against the fp64 oracle
(tests/gp_mlp_ref.py, with the kernels' codec ReLU decisions) and the reference's fp32 run; the fused training step
(eager and captured); the 64^2 and the nc = 16 factories; the surrogate predictor and the MC predictive with the MLP
map; and the guard that an L = 0 engine holds nothing of the new path."""
import numpy as np
import pytest
import torch

from test_gpu_parity import load, cuda, _DS
from test_gpu_c64 import check_mask_audit
from gp_mlp_ref import CASES, load_case, mlp, mlp_layers

pytestmark = pytest.mark.gpu


def mlp_model(d):
    """A fixture case's model on the GPU: test_gpu_parity.build_golden_model with the MLP map."""
    from bottleneck.Encoder import CNNEncoder
    from bottleneck.Decoder import CNNDecoder
    from bottleneck.components import EffectivePropertyMap, ReducedOrderModelOperator
    from bottleneck.ROM import ROM
    from bottleneck.generative import GenerativeModel
    from physics.grid import StructuredGrid
    n, nc, dz, Nu, bs, Ns = [int(v) for v in d['cfg']]
    enc = CNNEncoder(n, dz, [1, 1], 4, 4, drop_rate=0)
    dec = CNNDecoder(n, dz, (8, 8), 1, 4, [1, 1], False, 4, drop_rate=0.)
    rom = ROM(StructuredGrid(nc), n // nc)
    g = ReducedOrderModelOperator(rom, torch.tensor(d['W']), dtype=torch.float32, device='cuda')
    gp = EffectivePropertyMap(dz, 2 * nc * nc, num_hidden_layers=int(d['L']), independent_X=bool(int(d['independent_X'])),
                              dtype=torch.float32, device='cuda')
    model = GenerativeModel(f=dec.cuda(), g=g, gp=gp, dtype=torch.float32, device=torch.device('cuda'))
    model.encoder = enc.cuda()
    ds_s = _DS(X=cuda(d['Xs']), Y=cuda(d['Y']), F_ROM_BC=cuda(d['F']))
    ds_u = _DS(perm=torch.tensor(d['perm'], device='cuda'), X=cuda(d['Xu']))
    model.register_datasets({'supervised': ds_s, 'unsupervised': ds_u}, None,
                            create_unsupervised_variational_approximation=False)
    state = {k[6:]: torch.tensor(v) for k, v in d.items() if k.startswith('state.')}
    if not int(d['independent_X']):     # lock-X: no q_X rows, no gp.logsigmas_X
        state = {k: v for k, v in state.items() if not k.startswith('q_X.') and k != 'gp.logsigmas_X'}
    model.load_state_dict(state)
    model.cuda()
    return model, bs


def case_eps(d):
    ez = torch.cat([cuda(d['eps_enc']), cuda(d['eps_qz'])])
    return (ez, cuda(d['eps_qX'])) if int(d['independent_X']) else (ez,)


@pytest.mark.parametrize('normalize', [False, True], ids=['sum', 'normalize'])
@pytest.mark.parametrize('tag', CASES)
def test_mlp_elbo_module_path_c32(device, tag, normalize):
    """model.elbo + backward on a fixture case's inputs and noise: vs the fp64 oracle with the kernels' codec ReLU
    decisions at 1e-5 (value) and 5e-5 per gradient tensor; vs the reference's fp32 run at 2e-5 (value)."""
    from gp_mlp_ref import oracle_gpmlp_fixture_elbo
    from elbo_ref import tensor_rel
    from gpu_masks import engine_relu_masks
    from oracle import codec as ocodec
    d = load_case(tag)
    model, bs = mlp_model(d)
    elbo = model.elbo(step=0, armortized_bs=bs, eps=case_eps(d), normalize=normalize)
    (-elbo).backward()
    torch.cuda.synchronize()
    engine = model._elbo_engine(bs, int(d['cfg'][5]), normalize)
    L = int(d['L'])
    assert engine.gp_hidden == L and engine.gp_mlp_launches == 2 and len(engine.gp_mlp_buffers) == 2 * L
    assert engine.lockx == (not int(d['independent_X']))
    ocodec.MASK_AUDIT.clear()
    terms = {}
    val_o, gr_o = oracle_gpmlp_fixture_elbo(d, masks=engine_relu_masks(engine), terms=terms, normalize=normalize)
    check_mask_audit()
    assert terms['preact_min'] >= 1e-4
    errs = {k: tensor_rel(p.grad.cpu().numpy(), gr_o[k]) for k, p in model.named_parameters()}
    print('%s elbo %.6f oracle %.6f reference %.6f worst gradient tensor %.2e' % (
        tag, elbo.item(), val_o, float(d['elbo']), max(errs.values())))
    assert abs(elbo.item() - val_o) <= 1e-5 * abs(val_o), (elbo.item(), val_o)
    bad = {k: e for k, e in errs.items() if not e <= 5e-5}
    assert not bad, bad
    if not normalize:
        assert abs(elbo.item() - float(d['elbo'])) <= 2e-5 * abs(float(d['elbo'])), (elbo.item(), float(d['elbo']))
        t = engine.terms()
        for k in [k[len('term.objective/'):] for k in d if k.startswith('term.objective/') and not k.endswith('_elbo')]:
            assert abs(t[k] - float(d['term.objective/' + k])) <= 2e-5 * abs(float(d['term.objective/' + k])), k


def _step(d, model, bs, **kw):
    from gpi.train import FusedElboStep
    kw.setdefault('lr', 1e-3)
    kw.setdefault('seed', 7)
    return FusedElboStep(model, cuda(d['Xu']), bs, cuda(d['Xs']), cuda(d['Y']), cuda(d['F']), **kw)


def step_vs_module(step, model, ref_model, bs, rounds):
    """forward_backward() of a fused step against ref_model.elbo + backward on the step's own subset and noise:
    ELBO 1e-5 relative, every gradient tensor within 1e-4 of its max; update() between the rounds."""
    e = step.engine
    for it in range(rounds):
        with torch.no_grad():
            for (k, p), (k2, q) in zip(model.named_parameters(), ref_model.named_parameters()):
                assert k == k2
                q.copy_(p)
        eps = (e.eps_z().clone(),) + (() if e.lockx else (e.eps_x().clone(),))
        if e.has_dropout:
            drop = {k: {n: v.clone() for n, v in dd.items()} for k, dd in e.dropout_views().items()}
        ref_model._datasets['unsupervised'].perm = step.idx.clone().long()
        ref_model.zero_grad()
        ref = ref_model.elbo(step=it, armortized_bs=bs, eps=eps, **(dict(dropout=drop) if e.has_dropout else {}))
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
            if k.startswith('gp.fc.'):
                assert ref_g.abs().max().item() > 0, k
        step.update()
    torch.cuda.synchronize()
    step.check_handoff()
    step.engine.check_flag()


@pytest.mark.parametrize('tag', CASES)
def test_mlp_fused_step_matches_module_path(device, tag):
    d = load_case(tag)
    model, bs = mlp_model(d)
    ref_model, _ = mlp_model(d)
    step = _step(d, model, bs)
    assert step.engine.gp_hidden == int(d['L'])
    # the MLP's 2-D weights sit in the shared prefix of the flat buffer, 16-byte aligned
    for k, p in model.named_parameters():
        if k.startswith('gp.fc.') and p.dim() == 2:
            o = step.flat.name_offsets[k]
            assert o % 4 == 0 and o + p.numel() <= step.flat.n_shared, k
    step_vs_module(step, model, ref_model, bs, rounds=2)


@pytest.mark.parametrize('tag', ['fx2', 'lx1'])
def test_mlp_captured_step_replays_eager_bitwise(device, tag):
    """A captured step against an eager twin over 3 steps: parameters and ELBO bit for bit."""
    d = load_case(tag)
    model_a, bs = mlp_model(d)
    model_b, _ = mlp_model(d)
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


def _factory_models(identifier, Nu, Ns, seed, **opts):
    """Two identical factory models (random init, synthetic data) on the GPU with L = 1 -> (models, data, bs)."""
    from factories.model import ModelFactory
    from test_gpu_c64 import _DS as DS64
    out = []
    rng = np.random.default_rng(seed)
    data = None
    for _ in range(2):
        torch.manual_seed(seed)
        fac = ModelFactory.FromIdentifier(identifier, eff_property_map_hidden_layers=1, **opts)
        fac.set('device', 'cuda')
        physics_, model, _, encoder, _, _ = fac.setup()
        model.encoder = encoder.cuda()
        n, nc = physics_['fom'].grid.n, physics_['rom'].grid.n
        if data is None:
            Xu = rng.normal(0.3, 0.6, (Nu, n, n)).astype(np.float32)
            Xs = rng.normal(0.3, 0.6, (Ns, n, n)).astype(np.float32)
            Y = rng.normal(0.0, 0.3, (Ns, (n + 1) * (n - 1))).astype(np.float32)
            F = np.zeros((Ns, (nc + 1) ** 2), dtype=np.float32)
            bnodes = [e for e in range((nc + 1) ** 2) if e % (nc + 1) in (0, nc)]
            F[:, bnodes] = rng.uniform(-0.5, 0.5, (Ns, len(bnodes)))
            data = dict(Xu=Xu, Xs=Xs, Y=Y, F=F)
        model.register_datasets({'supervised': DS64(X=cuda(data['Xs']), Y=cuda(data['Y']), F_ROM_BC=cuda(data['F'])),
                                 'unsupervised': DS64(perm=torch.arange(Nu, device='cuda'), X=cuda(data['Xu']))}, None,
                                create_unsupervised_variational_approximation=False)
        model.cuda()
        out.append(model)
    return out, data


@pytest.mark.parametrize('identifier,widths,Nu,bs,Ns,opts', [
    ('highres', [64, 96, 128], 16, 8, 4, dict(droprate=0.2)),
    ('highres128_rom16', [64, 288, 512], 8, 4, 2, dict()),
], ids=['c64', 'c128_rom16'])
def test_mlp_fused_step_factories(device, identifier, widths, Nu, bs, Ns, opts):
    """One fused step vs the module path at the 64^2 codec (64 -> 96 -> 128, droprate 0.2) and at nc = 16
    (64 -> 288 -> 512: the layer that does not fit LDS)."""
    (model, ref_model), data = _factory_models(identifier, Nu, Ns, 23, **opts)
    assert model.gp.fc.widths == widths
    step = _step(data, model, bs)
    assert step.engine.gp_hidden == 1 and step.engine.gp_widths == widths
    step_vs_module(step, model, ref_model, bs, rounds=1)


def test_l0_engine_holds_nothing_of_the_mlp_path(device):
    """An L = 0 engine has no MLP launch and no h_k / delta_k buffer -- its workspace, head flags and GEMM items
    are the linear map's -- and its ELBO and flat gradient on elbo_c32.npz equal, bit for bit, those of a twin
    built without ever naming the option (test_gpu_parity.build_golden_model, which predates it; the other model
    passes num_hidden_layers = 0)."""
    from test_gpu_parity import build_golden_model
    d = load('elbo_c32.npz')
    eps = (torch.cat([cuda(d['eps_enc']), cuda(d['eps_qz'])]), cuda(d['eps_qX']))
    out = []
    for twin in (False, True):
        model, bs = build_golden_model(d) if twin else mlp_model(dict(d, L=0, independent_X=1))
        assert isinstance(model.gp.fc, torch.nn.Linear)
        engine = model._elbo_engine(bs, int(d['cfg'][5]), False)
        assert engine.gp_hidden == 0 and engine.gpm is None
        assert engine.gp_mlp_launches == 0 and engine.gp_mlp_buffers == {}
        assert len(engine.gemm_items) == 5 and engine.head.flags & 0x10          # GPI_HEAD_GP: the head's own product
        model.zero_grad()
        elbo = model.elbo(step=0, armortized_bs=bs, eps=eps)
        (-elbo).backward()
        torch.cuda.synchronize()
        out.append((elbo.item(), engine.flat.G.clone(), engine.ws.ws.size))
    assert out[0][0] == out[1][0] and torch.equal(out[0][1], out[1][1]) and out[0][2] == out[1][2]
    assert abs(out[0][0] - float(d['elbo'])) <= 2e-5 * abs(float(d['elbo']))


def _eval_stats(module, seed):
    gen = torch.Generator().manual_seed(seed)
    st = module.state_dict()
    for k, v in st.items():
        if k.endswith('running_mean'):
            st[k] = (0.5 * torch.randn(v.shape, generator=gen)).cuda()
        elif k.endswith('running_var'):
            st[k] = (0.5 + torch.rand(v.shape, generator=gen)).cuda()
    module.load_state_dict(st)


@pytest.mark.parametrize('B', [1, 5])
def test_surrogate_predictor_with_the_mlp_map(device, B):
    """SurrogatePredictor.predict with L = 1 vs fp64 eval-encoder mean -> MLP -> ROM at 1e-5 (relative to the
    prediction's max); the captured predictor equals the uncaptured one bit for bit."""
    import eval_ref
    from elbo_ref import tensor_rel
    from oracle import elbo as oelbo
    from gpi.infer import SurrogatePredictor
    d = load_case('fx1')
    model, _ = mlp_model(d)
    _eval_stats(model.encoder, 17)
    disc = model.extract_discriminative_model(FromLatentEncoding=False, duplicate=True)
    disc.eval()
    rng = np.random.default_rng(3)
    idx = rng.integers(0, len(d['Xu']), B)
    X = d['Xu'][idx]
    F = d['F'][rng.integers(0, len(d['F']), B)]
    p = SurrogatePredictor(disc, B)
    y0 = p.predict(cuda(X), cuda(F)).clone()
    n, nc, dz = [int(v) for v in d['cfg'][:3]]
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
    es = eval_ref.state64(dict(disc._encoder.state_dict()), '')
    mu, _ = eval_ref.encoder_eval(es, X, n, [1, 1], 4, 4)
    st = {'gp.fc.' + k: v.detach().double().cpu() for k, v in disc._gp.state_dict().items()}
    pre = []
    x_eff = mlp(mlp_layers(st), torch.as_tensor(mu, dtype=torch.float64), pre)
    assert min(float(a.abs().min()) for a in pre) > 1e-5
    y_ref = oelbo.rom_operator(t(d['W']), t(d['M']), torch.as_tensor(d['bc_dofs']), x_eff, t(F),
                               disc._g.logsigmas_y.detach().double().cpu())[0]
    assert tensor_rel(y0.cpu().numpy(), y_ref.numpy()) < 1e-5
    p.capture()
    assert torch.equal(p.replay(), y0)
    p.check_flag()


def test_predictive_y_with_the_mlp_map(device):
    """predictive_y (Analysis.eval_all_y's path) called directly with injected noise on the supervised q_z rows,
    against the fp64 restatement of the same draws (oracle.elbo.vo_predictive with the MLP as its map): free-X
    (with the logsigmas_X noise) at 1e-4, the bar of test_analysis_eval_all_y; lock-X (no X noise) at 1e-5.
    update_virtual_observables itself is test_lockx_vo_update_with_the_mlp_map."""
    from elbo_ref import tensor_rel
    from oracle import elbo as oelbo
    from gpi.predictive import predictive_y
    N_mc = 8
    for tag, tol in (('fx1', 1e-4), ('lx1', 1e-5)):
        d = load_case(tag)
        model, _ = mlp_model(d)
        lockx = not int(d['independent_X'])
        n, nc, dz, Nu, bs, Ns = [int(v) for v in d['cfg']]
        dx, dy = 2 * nc * nc, d['Y'].shape[1]
        rng = np.random.default_rng(31)
        ez = rng.normal(size=(Ns * N_mc, dz)).astype(np.float32)
        ex = rng.normal(size=(Ns * N_mc, dx)).astype(np.float32)
        ey = rng.normal(size=(Ns * N_mc, dy)).astype(np.float32)
        qz = model.q_z['supervised']
        mean, std = predictive_y(model, qz.mean.detach(), qz.logsigma.detach(), cuda(d['F']), N_mc,
                                 eps=(cuda(ez), None if lockx else cuda(ex), cuda(ey)))
        torch.cuda.synchronize()
        t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
        st = {k[6:]: t(v) for k, v in d.items() if k.startswith('state.')}
        layers = mlp_layers(st)
        pre = []
        if lockx:
            gp = lambda z: mlp(layers, z, pre)
        else:       # the logsigmas_X noise of the draws, row by row as vo_predictive calls the map
            ex_it = iter(t(ex).view(Ns, N_mc, dx))
            gp = lambda z: mlp(layers, z, pre) + torch.exp(st['gp.logsigmas_X']) * next(ex_it)
        Ym, Ys = oelbo.vo_predictive(t(d['W']), t(d['M']), torch.as_tensor(d['bc_dofs']), st['q_z.supervised._mean'],
                                     st['q_z.supervised._logsigma'], t(d['F']), st['g.logsigmas_y'],
                                     t(ez).view(Ns, N_mc, dz), t(ey).view(Ns, N_mc, dy), gp_linear=gp)
        assert min(float(a.abs().min()) for a in pre) > 1e-5
        assert tensor_rel(mean.cpu().numpy(), Ym.numpy()) < tol, tag
        assert tensor_rel(std.cpu().numpy(), Ys.numpy()) < tol, tag


# ---------------------------------------------------------------- the VO term
def _force_mlp_map(monkeypatch, L=1):
    """test_gpu_vo.build_vo_model constructs EffectivePropertyMap without the option: make it build L hidden layers."""
    import bottleneck.components as Cm
    real = Cm.EffectivePropertyMap

    def with_hidden(*a, **k):
        assert 'num_hidden_layers' not in k and len(a) <= 2
        return real(*a, num_hidden_layers=L, **k)

    monkeypatch.setattr(Cm, 'EffectivePropertyMap', with_hidden)


@pytest.mark.parametrize('holdoff', [False, True], ids=['active', 'holdoff'])
def test_mlp_fused_vo_step_matches_module_path(device, monkeypatch, holdoff):
    """The fused step with the VO term, N_vo = 4, L = 1 (16 -> 24 -> 32), active and held off, against the module
    path on the step's own subset and noise exactly as tests/test_gpu_fused_vo.py does it (its one_round: ELBO and
    the per-term VO values 1e-5, every gradient tensor within 1e-4 of its max, BN running buffers; two rounds with
    update() between them).  Active: the MLP launches run both q segments (N_s = 3 rows with lx_scale 1, then the 4
    VO rows with their own q rows and term slots); held off: the supervised rows only."""
    import test_gpu_fused_vo as fv
    import test_gpu_vo as tv
    from gp_mlp_ref import mlp_vo_fixture
    from gpi.train import VO_Y_SUB
    _force_mlp_map(monkeypatch)
    d = mlp_vo_fixture(tv.load('vo_elbo_c32.npz'), n_vo=4)
    Ns, Nvo = int(d['cfg'][5]), int(d['cfg'][6])
    assert Nvo == 4
    models = []
    for _ in range(2):
        model, ens, bs = tv.build_vo_model(d, independent_X=True)
        for it in range(2):
            model.update_virtual_observables(int(d['cfg'][7]), step=it, eps=fv.upd_eps(d, it))
        models.append((model, ens))
    (model, ens), (ref_model, _) = models
    assert model.gp.num_hidden_layers == 1 and model.gp.fc.widths == [16, 24, 32]
    step = fv.make_step(d, model, bs, vo_holdoff=holdoff)
    e = step.engine
    assert e.gp_hidden == 1 and e.gpm.n1 == Ns and e.gpm.n2 == (0 if holdoff else Nvo)
    assert len(e.roms) == (1 if holdoff else 2)
    y_draw = (step.rng_off.clone(), 100 + VO_Y_SUB)
    for it in range(2):
        off = step.rng_off.clone()
        fv.one_round(step, model, ref_model, ens, d, bs, False, holdoff, it, y_draw)
        y_draw = (off, VO_Y_SUB)
    G = step.flat.G
    for k, p in model.named_parameters():
        if k.startswith('gp.fc.'):
            o = step.flat.name_offsets[k]
            assert G[o:o + p.numel()].abs().max().item() > 0, k
    assert step.step_ctr.item() == 2
    step.check_handoff()
    step.engine.check_flag()


def test_lockx_vo_update_with_the_mlp_map(device, monkeypatch):
    """One lock-X GenerativeModel.update_virtual_observables with injected noise, N_mc = 8, L = 1, on
    vo_elbo_lockx_c32.npz's model with the MLP map: the MC predictive (y = g(mlp(z)), z ~ q_z['vo'], through
    gpi_gpmlp_sample) and the VO posterior it conditions, against the torch fp64 restatement of the same draws
    (oracle.elbo.vo_predictive / vo_condition, as elbo_ref.oracle_vo_updates composes them) at 1e-5 per tensor."""
    import test_gpu_vo as tv
    from elbo_ref import tensor_rel
    from gp_mlp_ref import mlp_vo_fixture
    from oracle import elbo as oelbo
    _force_mlp_map(monkeypatch)
    d = mlp_vo_fixture(tv.load('vo_elbo_lockx_c32.npz'))
    n, nc, dz, Nu, bs, Ns, Nvo, _ = [int(v) for v in d['cfg']]
    N_mc, dy = 8, d['Yv'].shape[1]
    model, ens, _ = tv.build_vo_model(d, independent_X=False)
    assert model.gp.num_hidden_layers == 1 and 'vo' not in model.q_X
    rng = np.random.default_rng(77)
    ez = rng.normal(size=(Nvo * N_mc, dz)).astype(np.float32)
    ey = rng.normal(size=(Nvo * N_mc, dy)).astype(np.float32)
    Ym, Ys = model.update_virtual_observables(N_mc, return_mean_stddev=True, step=0, eps=(cuda(ez), cuda(ey)))
    torch.cuda.synchronize()
    ens.check_flag()
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
    st = {k[6:]: t(v) for k, v in d.items() if k.startswith('state.') and np.asarray(v).dtype.kind == 'f'}
    layers, pre = mlp_layers(st), []
    W, M, bc = t(d['W']), t(d['M']), torch.as_tensor(d['bc_dofs'])
    Ym_o, Ys_o = oelbo.vo_predictive(W, M, bc, st['q_z.vo._mean'], st['q_z.vo._logsigma'], t(d['Fv']),
                                     st['g.logsigmas_y'], t(ez).view(Nvo, N_mc, dz), t(ey).view(Nvo, N_mc, dy),
                                     gp_linear=lambda z: mlp(layers, z, pre))
    assert min(float(a.abs().min()) for a in pre) > 1e-5
    G, A = t(d['Gamma']), t(d['alpha'])
    m = G.shape[1]
    infinite = torch.zeros(m, dtype=torch.bool)
    infinite[:(nc + 1) ** 2] = True
    vo_var = oelbo.vo_mean_variances(torch.ones(m, dtype=torch.float64), Nvo, infinite)
    res = [oelbo.vo_condition(G[i], A[i], Ym_o[i], 1 / Ys_o[i] ** 2, vo_var) for i in range(Nvo)]
    errs = dict(Y_mean=tensor_rel(Ym.cpu(), Ym_o), Y_std=tensor_rel(Ys.cpu(), Ys_o),
                mean=tensor_rel(ens.mean.cpu(), torch.stack([r[0] for r in res])),
                vars=tensor_rel(ens.vars.cpu(), torch.stack([r[1] for r in res])))
    print('lock-X VO update with the MLP map', errs)
    assert max(errs.values()) < 1e-5, errs
