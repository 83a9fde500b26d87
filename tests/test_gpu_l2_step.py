"""FusedElboStep(l2_penalty=): model.elbo's l2_penalty (generative.py:381-385) in the fused training step, on the C32
golden model of elbo_opts_c32.npz.

a. differential: a step with the penalty against a step without it, from the same model and seed: unpenalised
   gradient elements bit for bit, penalised ones G_A + lambda32 p / ||p||_64 within 4 * 2^-24 (|G_A| + |lambda p /
   ||p|||) -- one rounding each for the coefficient, the product and the sum --, elbo() less lambda * pen (1e-6).
b. the module path (GenerativeModel.elbo(l2_penalty=)) on the step's subset and noise: value 1e-6, every gradient
   tensor 1e-5 per-tensor relative (tests/test_gpu_c64.py::test_fused_step_c64's bars: the same kernels).
c. the fp64 oracle with the kernels' ReLU decisions: value 1e-5, every gradient tensor 5e-5.
d. three Adam steps in every step form, bit-identical to an eager twin; set_l2_penalty on a captured step.
e. l2_penalty=0.0 equals None (gradient, parameters, moments).   f. None launches nothing and carries NULL fields.
g. (a) on the highres C64 codec with dropout, captured, and on a homoscedastic C32 model (f.logsigma penalised).

The factor is chosen from a run without the penalty so that the penalty's gradient is visible beside every
penalised tensor's data gradient (the fixture's own 0.05 is lost beside C32 gradients of 1e2 .. 1e4)."""
import copy
import sys

import numpy as np
import pytest
import torch

from elbo_ref import load, oracle_elbo, tensor_rel, check_grads
from oracle import codec as ocodec

pytestmark = pytest.mark.gpu
sys.path.insert(0, __file__.rsplit('/', 1)[0])
U = 2.0 ** -24


def cuda(a, dtype=torch.float32):
    return torch.tensor(np.asarray(a), dtype=dtype, device='cuda')


def golden():
    from test_gpu_parity import build_golden_model
    d = load('elbo_opts_c32.npz')
    model, bs = build_golden_model(d)
    data = tuple(cuda(d[k]) for k in ('Xu', 'Xs', 'Y', 'F'))
    return d, model, bs, data


def make_step(model, bs, data, l2, **kw):
    from gpi.train import FusedElboStep
    Xu, Xs, Y, F = data
    kw.setdefault('lr', 1e-3)
    kw.setdefault('seed', 11)
    return FusedElboStep(model, Xu, bs, Xs, Y, F, l2_penalty=l2, **kw)


def rows_of(step):
    from gpi.train import l2_segments
    return l2_segments(step.model, step.flat)


def penalty_reference(P, rows, lam):
    """(dense fp64 lambda32 p / ||p||_64 over the flat buffer, penalised mask, pen, norms) from host parameters."""
    lam32 = float(np.float32(lam))
    P = np.asarray(P, dtype=np.float64)
    x = np.zeros(P.size)
    mask = np.zeros(P.size, dtype=bool)
    norms = []
    for _, o, n in rows:
        nv = float(np.sqrt(np.sum(P[o:o + n] ** 2)))
        norms.append(nv)
        mask[o:o + n] = True
        if nv > 0:
            x[o:o + n] = lam32 * P[o:o + n] / nv
    return x, mask, float(np.sum(norms)), np.array(norms)


def choose_lambda(G0, P, rows):
    """The smallest factor with lambda / sqrt(numel) >= 1e-3 max|G0| for every penalised tensor of non-zero norm
    (the penalty's gradient has 2-norm lambda, so its rms element is lambda / sqrt(numel))."""
    _, _, _, norms = penalty_reference(P, rows, 1.0)
    need = [1e-3 * np.abs(G0[o:o + n]).max() * np.sqrt(n) for (_, o, n), nv in zip(rows, norms) if nv > 0]
    lam = float(np.float32(max(need) * 1.01))
    for (_, o, n), nv in zip(rows, norms):
        if nv > 0:
            assert lam / np.sqrt(n) >= 1e-3 * np.abs(G0[o:o + n]).max()
    return lam


def differential(GA, GB, P0, rows, lam, elbo_a, elbo_b, terms_b, tag=''):
    GA64, GB64 = GA.astype(np.float64), GB.astype(np.float64)
    x, mask, pen, norms = penalty_reference(P0, rows, lam)
    assert (norms == 0).any() and (norms > 0).any(), 'the state needs a zero tensor and a non-zero one'
    assert np.array_equal(GA[~mask].view(np.uint32), GB[~mask].view(np.uint32)), 'an unpenalised element moved'
    assert np.isfinite(GB).all()
    err = np.abs(GB64 - (GA64 + x))[mask]
    bound = (4 * U * (np.abs(GA64) + np.abs(x)))[mask]
    ratio = (err[bound > 0] / bound[bound > 0]).max()
    print('%s lambda %.4g, pen %.6g: worst |G_B - (G_A + x)| / bound = %.3f' % (tag, lam, pen, ratio))
    assert (err <= bound).all(), ratio
    # not an empty check: the penalty moved every penalised tensor of non-zero norm, the zero ones not at all
    for (name, o, n), nv in zip(rows, norms):
        same = np.array_equal(GA[o:o + n], GB[o:o + n])
        assert same == (nv == 0), name
    lam32 = float(np.float32(lam))
    want = elbo_a - lam32 * pen
    assert abs(elbo_b - want) <= 1e-6 * abs(want), (elbo_b, want)
    assert abs(terms_b['elbo_l2_penalty'] - pen) <= 1e-6 * pen
    return x, mask, pen


@pytest.fixture(scope='module')
def base(device):
    """One step without the penalty on the fixture state: its gradient, parameters and value; the factor chosen
    from it.  Shared, never modified."""
    d, model, bs, data = golden()
    pristine = copy.deepcopy(model)
    A = make_step(model, bs, data, None)
    rows = rows_of(A)
    P0 = A.flat.P.cpu().numpy().copy()
    _, _, _, norms = penalty_reference(P0, rows, 1.0)
    if not (norms == 0).any():          # (the seeded init has all-zero BN biases; a trained state need not)
        name = next(n for n, _, _ in rows if 'norm' in n and n.endswith('.bias'))
        with torch.no_grad():
            dict(pristine.named_parameters())[name[:]].zero_()
        model = copy.deepcopy(pristine)
        A = make_step(model, bs, data, None)
        rows = rows_of(A)
        P0 = A.flat.P.cpu().numpy().copy()
    A.forward_backward()
    torch.cuda.synchronize()
    GA = A.flat.G.cpu().numpy().copy()
    lam = choose_lambda(GA, P0, rows)
    out = dict(d=d, pristine=pristine, bs=bs, data=data, rows=rows, P0=P0, GA=GA, lam=lam, elbo_a=A.elbo().item(),
               terms_a=A.terms())
    A.update()
    torch.cuda.synchronize()
    return out


def fresh(base, l2, **kw):
    return make_step(copy.deepcopy(base['pristine']), base['bs'], base['data'], l2, **kw)


def test_differential_value_module_path_and_oracle(base):
    """(a), (b) and (c) on one step with the penalty."""
    from gpu_masks import engine_relu_masks
    from test_gpu_c64 import check_mask_audit
    d, bs, lam = base['d'], base['bs'], base['lam']
    assert 'elbo_l2_penalty' not in base['terms_a']
    B = fresh(base, lam)
    ref_model = copy.deepcopy(base['pristine'])
    assert np.array_equal(B.flat.P.cpu().numpy(), base['P0'])
    e = B.engine
    eps_z_t, eps_x_t = e.eps_z().clone(), e.eps_x().clone()
    idx_t = B.idx.clone().long()
    B.forward_backward()
    torch.cuda.synchronize()
    GB = B.flat.G.cpu().numpy().copy()
    # ---- a
    differential(base['GA'], GB, base['P0'], base['rows'], lam, base['elbo_a'], B.elbo().item(), B.terms(), 'c32')
    # ---- b: the module path on the step's own subset and noise
    lam32 = float(np.float32(lam))
    ref_model._datasets['unsupervised'].perm = idx_t
    ref_model.zero_grad()
    ref = ref_model.elbo(step=0, armortized_bs=bs, eps=(eps_z_t, eps_x_t), l2_penalty=lam32)
    (-ref).backward()
    got = B.elbo().item()
    assert abs(got - ref.item()) <= 1e-6 * abs(ref.item()), (got, ref.item())
    off = B.flat.name_offsets
    G = B.flat.G
    g_of = lambda k, p: G[off[k]:off[k] + p.numel()].cpu().numpy().reshape(tuple(p.shape))
    errs_mod = {k: tensor_rel(g_of(k, p), p.grad.cpu().numpy()) for k, p in ref_model.named_parameters()}
    bad = {k: v for k, v in errs_mod.items() if not v < 1e-5}
    assert not bad, bad
    # ---- c: the fp64 oracle with the kernels' ReLU decisions
    n, nc = int(d['cfg'][0]), int(d['cfg'][1])
    st = {k: torch.tensor(p.detach().cpu().numpy(), dtype=torch.float64, requires_grad=True)
          for k, p in ref_model.named_parameters()}
    masks = engine_relu_masks(ref_model._elbo_engine(bs, int(d['cfg'][5]), False))
    eps_z = eps_z_t.cpu().numpy().astype(np.float64)
    idx = idx_t.cpu().numpy()
    ocodec.MASK_AUDIT.clear()
    val = oracle_elbo(st, d['Xu'][idx], d['Xs'], d['Y'], d['F'], eps_z[:bs], eps_z[bs:],
                      eps_x_t.cpu().numpy().astype(np.float64), nc, n // nc, masks=masks, l2_penalty=lam32)
    check_mask_audit()
    (-val).backward()
    assert abs(got - val.item()) <= 1e-5 * abs(val.item()), (got, val.item())
    errs = {k: tensor_rel(g_of(k, st[k]), st[k].grad.numpy()) for k in st}
    print(check_grads(errs, tol_all=5e-5, frac_tight=1.0))
    B.update()
    torch.cuda.synchronize()


def state_of(step):
    torch.cuda.synchronize()
    return [step.flat.P.clone(), step.m.clone(), step.v.clone(), step.elbo().clone()]


def assert_same(a, b, what):
    for k, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), (what, ('P', 'm', 'v', 'elbo')[k])
    assert a[0].view(torch.int32).eq(b[0].view(torch.int32)).all(), what


@pytest.fixture(scope='module')
def eager_twin(base):
    """Eager steps with the penalty (the fused epilogue + Adam launch): the state after 3 and after 4 steps."""
    T = fresh(base, base['lam'])
    assert T.fuse_adam
    states = {}
    for k in range(1, 5):
        T.step()
        if k >= 3:
            states[k] = state_of(T)
    assert not torch.equal(states[3][0], torch.tensor(base['P0'], device='cuda'))
    return states


@pytest.mark.parametrize('form', ['fb_update', 'two_launch_adam', 'streams', 'single', 'unroll2'])
def test_three_steps_bit_identical_in_every_form(base, eager_twin, form, monkeypatch):
    """(d): parameters, Adam moments and elbo() after three steps (unroll: run(4) against four) equal the eager
    twin's bit for bit."""
    lam = base['lam']
    if form == 'two_launch_adam':
        monkeypatch.setenv('GPI_FUSED_ADAM', '0')      # (read by every constructor, not once per process)
    if form in ('streams', 'single'):
        monkeypatch.setenv('GPI_GRAPH_MODE', form)
    S = fresh(base, lam)
    n = 3
    if form == 'fb_update':
        for _ in range(3):
            S.forward_backward()
            S.update()
            S.engine.rejoin()
    elif form == 'two_launch_adam':
        assert not S.fuse_adam
        for _ in range(3):
            S.step()
    elif form in ('streams', 'single'):
        S.capture()
        if S.graph_mode != form:
            assert form == 'streams' and S.graph_mode == 'single', 'only the queue probe may change the mode'
        for _ in range(3):
            S.step()
    else:
        S.capture(unroll=2)
        S.run(4)
        n = 4
    assert_same(state_of(S), eager_twin[n], form)
    S.check_handoff()
    assert int(S.step_ctr.item()) == n


def test_set_l2_penalty_reaches_a_captured_step(base, eager_twin):
    """(d, last item): after set_l2_penalty(2 lambda) the next replay's gradient is the one of an eager twin stepped
    with 2 lambda from the start of that step, and lies the extra lambda p / ||p|| above the lambda twin's."""
    lam, rows = base['lam'], base['rows']
    S, T2, T1 = fresh(base, lam), fresh(base, lam), fresh(base, lam)
    S.capture()
    for _ in range(3):
        S.step()
        T2.step()
        T1.step()
    assert_same(state_of(S), eager_twin[3], 'captured')
    P3 = S.flat.P.cpu().numpy().copy()
    S.set_l2_penalty(2 * lam)
    T2.set_l2_penalty(2 * lam)
    for s in (S, T2, T1):
        s.step()
    torch.cuda.synchronize()
    assert torch.equal(S.flat.G, T2.flat.G) and torch.equal(S.flat.P, T2.flat.P)
    assert torch.equal(S.elbo(), T2.elbo())
    G2, G1 = S.flat.G.cpu().numpy(), T1.flat.G.cpu().numpy()
    x, mask, pen, _ = penalty_reference(P3, rows, lam)
    assert np.array_equal(G2[~mask], G1[~mask])
    err = np.abs(G2.astype(np.float64) - (G1.astype(np.float64) + x))[mask]
    bound = (4 * U * (np.abs(G1.astype(np.float64)) + np.abs(x)))[mask]
    assert (err <= bound).all(), (err[bound > 0] / bound[bound > 0]).max()
    assert not np.array_equal(G2[mask], G1[mask])
    assert abs(S.terms()['elbo_l2_penalty'] - pen) <= 1e-6 * pen
    with pytest.raises(Exception, match='l2_penalty=None'):
        fresh(base, None).set_l2_penalty(1.0)


def test_zero_penalty_equals_none(base):
    """(e)"""
    N, Z = fresh(base, None), fresh(base, 0.0)
    assert Z.l2 is not None and float(Z.l2.item()) == 0.0
    for _ in range(3):
        N.step()
        Z.step()
    torch.cuda.synchronize()
    for a, b in ((N.flat.G, Z.flat.G), (N.flat.P, Z.flat.P), (N.m, Z.m), (N.v, Z.v), (N.elbo(), Z.elbo())):
        assert torch.equal(a, b)
    assert 'elbo_l2_penalty' in Z.terms() and Z.terms()['elbo_l2_penalty'] > 0
    assert 'elbo_l2_penalty' not in N.terms()


def test_default_step_launches_no_norms(base, monkeypatch):
    """(f): counted through the binding's one call site."""
    from gpi import train
    calls = []
    real = train.param_norms
    monkeypatch.setattr(train, 'param_norms', lambda desc, st: (calls.append(1), real(desc, st))[1])
    N = fresh(base, None)
    assert N.l2 is None
    for epi in (N.epi, N.epi_adam):
        assert epi.pen_grad is None and epi.pen_src is None and epi.pen_dst is None and epi.pen_n == 0
    N.step()
    N.forward_backward()
    N.update()
    N.engine.rejoin()
    N.capture()
    N.step()
    torch.cuda.synchronize()
    assert calls == []
    B = fresh(base, base['lam'])
    for epi in (B.epi, B.epi_adam):
        assert epi.pen_grad == B.pen_grad.data_ptr() and epi.pen_n == B.pen_n
    B.step()
    B.step()
    torch.cuda.synchronize()
    assert len(calls) == 2                          # one launch per step


def synthetic(ident, n, Nu, Ns, seed, droprate=None, **factory_kw):
    from factories.model import ModelFactory
    from test_gpu_c64 import _DS
    torch.manual_seed(seed)
    fac = ModelFactory.FromIdentifier(ident, **factory_kw)
    fac.set('device', 'cuda')
    if droprate is not None:
        fac.set('droprate', droprate)
    physics_, model, _, encoder, _, _ = fac.setup()
    model.encoder = encoder.cuda()
    nc = physics_['rom'].grid.n
    assert physics_['fom'].grid.n == n
    rng = np.random.default_rng(seed)
    Xu = rng.normal(0.3, 0.6, (Nu, n, n)).astype(np.float32)
    Xs = rng.normal(0.3, 0.6, (Ns, n, n)).astype(np.float32)
    Y = rng.normal(0.0, 0.3, (Ns, (n + 1) * (n - 1))).astype(np.float32)
    F = np.zeros((Ns, (nc + 1) ** 2), dtype=np.float32)
    bnodes = [e for e in range((nc + 1) ** 2) if e % (nc + 1) in (0, nc)]
    F[:, bnodes] = rng.uniform(-0.5, 0.5, (Ns, len(bnodes)))
    model.register_datasets({'supervised': _DS(X=cuda(Xs), Y=cuda(Y), F_ROM_BC=cuda(F)),
                             'unsupervised': _DS(perm=torch.arange(Nu, device='cuda'), X=cuda(Xu))}, None,
                            create_unsupervised_variational_approximation=False)
    model.cuda()
    return model, (cuda(Xu), cuda(Xs), cuda(Y), cuda(F))


@pytest.mark.parametrize('case', ['highres-c64-dropout', 'homoscedastic-c32'])
def test_differential_on_other_codecs(device, case):
    """(g): (a) on one captured step of the highres C64 codec (B_u = 8 of 16, N_s = 4, droprate 0.2) and of a
    homoscedastic C32 model, whose noise plane f.logsigma is a penalised tensor (all zero at init: gradient
    unchanged; so the plane is set to a non-zero constant here and its gradient carries the penalty)."""
    if case == 'highres-c64-dropout':
        model, data = synthetic('highres', 64, 16, 4, seed=7, droprate=0.2)
        bs = 8
    else:
        model, data = synthetic('highres32', 32, 16, 4, seed=9, homoscedastic=True)
        bs = 8
        with torch.no_grad():
            model.f.logsigma.fill_(-0.5)
    models = [model, copy.deepcopy(model)]
    A = make_step(models[0], bs, data, None, seed=5)
    rows = rows_of(A)
    P0 = A.flat.P.cpu().numpy().copy()
    A.capture()
    A.step()
    torch.cuda.synchronize()
    GA = A.flat.G.cpu().numpy().copy()
    lam = choose_lambda(GA, P0, rows)
    B = make_step(models[1], bs, data, lam, seed=5)
    assert np.array_equal(B.flat.P.cpu().numpy(), P0)
    if case == 'highres-c64-dropout':
        assert B.engine.dropout_views()
    B.capture()
    B.step()
    torch.cuda.synchronize()
    GB = B.flat.G.cpu().numpy().copy()
    differential(GA, GB, P0, rows, lam, A.elbo().item(), B.elbo().item(), B.terms(), case)
    if case == 'homoscedastic-c32':
        name, o, n = next(r for r in rows if r[0] == 'f.logsigma')
        assert n == 32 * 32 and not np.array_equal(GA[o:o + n], GB[o:o + n])
    A.check_handoff()
    B.check_handoff()
