"""Partially observed labels through the ELBO: model.preprocess_y_fct = ObservedDofs(idx) and
model.set_label_mask(mask) on the module path (GenerativeModel.elbo) and in FusedElboStep, eager and captured.

The C32 fixture elbo_partial_c32.npz is the reference's own run with preprocess_y_fct = lambda y: y[..., idx]
(128 of 1023 nodes): ELBO 1e-5 against the fp64 restatement (tests/partial_ref.py) with the kernels' ReLU
decisions, every gradient tensor 5e-5 (max|g - ref| / max|ref|, no floor), 2e-5 against the reference's value.
The unobserved entries of Y hold NaN in every masked run here: they are never read into a result."""
import copy
import functools

import numpy as np
import pytest
import torch

from elbo_ref import tensor_rel, check_grads
from gpu_masks import engine_relu_masks
from test_gpu_parity import load, build_golden_model, cuda
import partial_ref as P

pytestmark = pytest.mark.gpu
D_Y = 1023


@functools.lru_cache(maxsize=None)
def fixture():
    return load('elbo_partial_c32.npz')


def holes(d, w):
    """The fixture with NaN at every unobserved label entry (w [d_y] or [N_s, d_y])."""
    d = dict(d)
    Y = d['Y'].copy()
    Y[np.broadcast_to(w, Y.shape) == 0] = np.nan
    d['Y'] = Y
    return d


def eps_of(d, lockx=False):
    return (torch.cat([cuda(d['eps_enc']), cuda(d['eps_qz'])]), None if lockx else cuda(d['eps_qX']))


def observed(d):
    from bottleneck.utils import ObservedDofs
    return ObservedDofs(d['idx'])


def per_sample_mask(d, seed=3):
    """[N_s, d_y]: another 25 % of the nodes per labelled sample."""
    return (np.random.default_rng(seed).random((int(d['cfg'][5]), D_Y)) < 0.25).astype(np.float32)


def grads_of(model):
    return {k: p.grad.detach().cpu().numpy() for k, p in model.named_parameters()}


# ---------------------------------------------------------------- the C32 fixture, module path
def test_fixture_through_model_elbo(device):
    d0 = fixture()
    w = P.index_weights(d0['idx'], D_Y)
    d = holes(d0, w)
    model, bs = build_golden_model(d)
    model.preprocess_y_fct = observed(d)
    elbo = model.elbo(step=0, armortized_bs=bs, eps=eps_of(d))
    (-elbo).backward()
    engine = model._elbo_engine(bs, int(d['cfg'][5]), False)
    assert engine.rom.y_weight == model.label_weights().data_ptr() and engine.rom.yw_stride == 0
    val_o, gr_o = P.oracle_partial_fixture_elbo(d, w, masks=engine_relu_masks(engine))
    e_ref = abs(elbo.item() - float(d['elbo'])) / abs(float(d['elbo']))
    e_o = abs(elbo.item() - val_o) / abs(val_o)
    print('elbo %.6f | restatement %.6f (%.2e) | reference %.6f (%.2e)' % (elbo.item(), val_o, e_o, float(d['elbo']), e_ref))
    assert e_o <= 1e-5
    assert e_ref < 2e-5
    terms = engine.terms()
    ref_ll = float(d['term.objective/supervised_logL_y'])
    assert abs(terms['supervised_logL_y'] - ref_ll) <= 2e-5 * abs(ref_ll)
    print(check_grads({k: tensor_rel(g, gr_o[k]) for k, g in grads_of(model).items()}, tol_all=5e-5, frac_tight=1.0))
    # no VO term: exactly no gradient to logsigma_y at nodes that no labelled sample observes
    gls = model.g.logsigmas_y.grad.cpu().numpy()
    assert np.all(gls[w == 0] == 0) and np.all(gls[w == 1] != 0)
    # elbo_supervised takes the same route
    model.zero_grad()
    sup = model.elbo_supervised(cuda(d['Xs']), cuda(d['Y']), step=0)
    assert torch.isfinite(sup)


def test_lockx_and_per_sample_masks_against_the_restatement(device):
    d0 = fixture()
    for lockx, kind in ((True, 'index'), (False, 'mask'), (True, 'mask')):
        w = P.index_weights(d0['idx'], D_Y) if kind == 'index' else per_sample_mask(d0)
        d = holes(d0, w)
        model, bs = build_golden_model(d, independent_X=not lockx)
        if kind == 'index':
            model.preprocess_y_fct = observed(d)
        else:
            model.set_label_mask(cuda(w) > 0)                    # a bool mask is converted once
        elbo = model.elbo(step=0, armortized_bs=bs, eps=eps_of(d, lockx))
        (-elbo).backward()
        engine = model._elbo_engine(bs, int(d['cfg'][5]), False)
        assert engine.lockx == lockx and engine.rom.yw_stride == (0 if kind == 'index' else D_Y)
        val_o, gr_o = P.oracle_partial_fixture_elbo(d, w, masks=engine_relu_masks(engine), lockx=lockx)
        e_o = abs(elbo.item() - val_o) / abs(val_o)
        print('lockx %s %s: elbo %.6f restatement %.6f (%.2e)' % (lockx, kind, elbo.item(), val_o, e_o))
        assert e_o <= 1e-5
        print(check_grads({k: tensor_rel(g, gr_o[k]) for k, g in grads_of(model).items()}, tol_all=5e-5,
                          frac_tight=1.0))
        seen = np.broadcast_to(w, (int(d['cfg'][5]), D_Y)).any(0)
        gls = model.g.logsigmas_y.grad.cpu().numpy()
        assert np.all(gls[~seen] == 0) and np.all(gls[seen] != 0)


def test_default_model_launches_what_it_launched_before(device):
    """No mask: the descriptor's y_weight is NULL, and a model that had a mask set and cleared gives the bits of
    one that never had any (fresh engine per mask; the unmasked engine is the one built before)."""
    d = load('elbo_c32.npz')
    model, bs = build_golden_model(d)
    never = copy.deepcopy(model)
    eps = eps_of(d)
    Ns = int(d['cfg'][5])

    def run(m):
        m.zero_grad()
        e = m.elbo(step=0, armortized_bs=bs, eps=eps)
        (-e).backward()
        return e.detach().clone(), [p.grad.clone() for p in m.parameters()]

    e0, g0 = run(never)
    eng0 = never._elbo_engine(bs, Ns, False)
    assert eng0.rom.y_weight is None and eng0.rom.yw_stride == 0 and eng0.y_weight is None
    e1, g1 = run(model)
    plain_engine = model._elbo_engine(bs, Ns, False)
    model.set_label_mask(torch.ones(Ns, D_Y, device='cuda'))
    e2, g2 = run(model)
    assert model._elbo_engine(bs, Ns, False) is not plain_engine
    assert model._elbo_engine(bs, Ns, False).rom.yw_stride == D_Y
    model.set_label_mask(None)
    assert model._elbo_engine(bs, Ns, False) is plain_engine and plain_engine.rom.y_weight is None
    e3, g3 = run(model)
    names = [k for k, _ in model.named_parameters()]
    for tag, e, g in (('first', e1, g1), ('all-ones mask', e2, g2), ('cleared', e3, g3)):
        assert torch.equal(e, e0), tag                    # (all-ones weights change nothing either)
        diff = [(k, (a - b).abs().max().item()) for k, a, b in zip(names, g, g0) if not torch.equal(a, b)]
        assert not diff, (tag, diff)


# ---------------------------------------------------------------- the fused step
def make_step(d, model, bs, **kw):
    from gpi.train import FusedElboStep
    return FusedElboStep(model, cuda(d['Xu']), bs, cuda(d['Xs']), cuda(d['Y']), cuda(d['F']), lr=1e-3, seed=7, **kw)


def test_fused_step_eager_and_captured(device):
    """FusedElboStep takes the mask from the model at construction.  One step against the module path on the
    step's own subset and noise (the bars of test_fused_step_matches_module_path), then three steps eager
    beside three replays of the captured step from the same state: parameters, gradient, Adam moments and
    ELBO terms equal bit for bit between the two forms."""
    d0 = fixture()
    w = P.index_weights(d0['idx'], D_Y)
    d = holes(d0, w)
    model, bs = build_golden_model(d)
    model.preprocess_y_fct = observed(d)
    ref_model = copy.deepcopy(model)
    twin = copy.deepcopy(model)
    assert isinstance(ref_model.preprocess_y_fct, type(model.preprocess_y_fct))
    step = make_step(d, model, bs)
    assert step.engine.rom.y_weight == model.label_weights().data_ptr()
    e = step.engine
    eps = (e.eps_z().clone(), e.eps_x().clone())
    ref_model._datasets['unsupervised'].perm = step.idx.clone().long()
    ref = ref_model.elbo(step=0, armortized_bs=bs, eps=eps)
    (-ref).backward()
    step.forward_backward()
    torch.cuda.synchronize()
    assert abs(step.elbo().item() - ref.item()) <= 1e-5 * abs(ref.item()), (step.elbo().item(), ref.item())
    for k, p in ref_model.named_parameters():
        g = step.flat.G[step.flat.name_offsets[k]:step.flat.name_offsets[k] + p.numel()].view(p.shape)
        err = (g - p.grad).abs().max().item() / max(p.grad.abs().max().item(), 1.0)
        assert err < 1e-4, (k, err)
    o = step.flat.offset(model.g.logsigmas_y)
    gls = step.flat.G[o:o + D_Y].cpu().numpy()
    assert np.all(gls[w == 0] == 0) and np.all(gls[w == 1] != 0)
    step.update()
    torch.cuda.synchronize()
    # eager beside captured, from the same state (twin: the model before any step)
    eager = make_step(d, twin, bs)
    graph_model = copy.deepcopy(twin)
    graph = make_step(d, graph_model, bs)
    graph.capture()
    assert graph.graph is not None
    for it in range(3):
        eager.step()
        graph.step()
        torch.cuda.synchronize()
        for name, a, b in (('P', eager.flat.P, graph.flat.P), ('G', eager.flat.G, graph.flat.G), ('m', eager.m, graph.m),
                           ('v', eager.v, graph.v), ('terms', eager.last_terms, graph.last_terms)):
            assert torch.equal(a, b), (it, name, (a - b).abs().max().item())
    assert torch.isfinite(graph.flat.P).all() and graph.step_ctr.item() == 3


def test_in_place_mask_edit_and_replaced_mask(device):
    """The captured step holds the mask tensor's address, not its contents.  c is captured on mask A; edited in
    place to B before its first replay it takes the first step of b (built and captured on B), not a's (on A);
    edited back to A between its first and second replay it takes the two steps of an eager step object whose
    mask went B, then A.  Replacing or clearing the model's mask raises at the next step."""
    from gpi import _lib as L
    d0 = fixture()
    w_a, w_b = per_sample_mask(d0, 3), per_sample_mask(d0, 4)
    d = holes(d0, np.maximum(w_a, w_b))                           # NaN where neither mask observes
    base, bs = build_golden_model(d)
    models = [copy.deepcopy(base) for _ in range(4)]
    masks = [cuda(w_a), cuda(w_b), cuda(w_a), cuda(w_b)]
    for m, t in zip(models, masks):
        m.set_label_mask(t)
        assert m.label_weights().data_ptr() == t.data_ptr()       # contiguous fp32: kept as it is
    a, b, c, e = [make_step(d, m, bs) for m in models]
    for s in (a, b, c):
        s.capture()
        assert s.graph is not None
    state = lambda s: (s.last_terms.clone(), s.flat.G.clone(), s.flat.P.clone())
    eq = lambda x, y: all(torch.equal(p, q) for p, q in zip(x, y))
    masks[2].copy_(masks[1])                                      # c: A -> B, before the first replay
    for s in (a, b, c, e):
        s.step()
    torch.cuda.synchronize()
    assert eq(state(c), state(b)) and not eq(state(c), state(a))
    assert eq(state(e), state(b))                                 # (eager and captured take the same step)
    masks[2].copy_(cuda(w_a))                                     # c and e: B -> A, between two replays
    masks[3].copy_(cuda(w_a))
    for s in (b, c, e):
        s.step()
    torch.cuda.synchronize()
    assert eq(state(c), state(e)) and not eq(state(c), state(b))
    models[2].set_label_mask(cuda(w_a))                           # another tensor: the step reads the old one
    with pytest.raises(L.NativeError, match='label mask'):
        c.step()
    models[2].set_label_mask(None)
    with pytest.raises(L.NativeError, match='label mask'):
        c.run(1)
    with pytest.raises(ValueError):                               # not the registered labels' shape
        models[2].set_label_mask(torch.ones(int(d['cfg'][5]) + 1, D_Y, device='cuda'))


# ---------------------------------------------------------------- with the VO term
def test_vo_term_stays_unmasked(device):
    """N_vo = 4 active beside a masked supervised term: the VO launch carries no weights, the ELBO and every
    gradient match the restatement (weights on the supervised term only), and logsigma_y's gradient at the
    nodes that no labelled sample observes is the VO launch's contribution."""
    from test_gpu_vo import build_vo_model
    from test_gpu_vo import load as load_vo
    from bottleneck.utils import ObservedDofs
    d = P.vo_fixture(load_vo('vo_elbo_c32.npz'), n_vo=4)
    n, nc, dz, Nu, bs, Ns, Nvo, Nmc = [int(v) for v in d['cfg']]
    assert Nvo == 4
    idx = np.sort(np.random.default_rng(9).choice(D_Y, 128, replace=False))
    w = P.index_weights(idx, D_Y)
    Ys = d['Ys'].copy()
    Ys[:, w == 0] = np.nan
    d['Ys'] = Ys
    model, ens, bs = build_vo_model(d)
    model.preprocess_y_fct = ObservedDofs(idx)
    for it in range(2):
        model.update_virtual_observables(Nmc, step=it, eps=(cuda(d['upd%d.eps_X' % it]), cuda(d['upd%d.eps_y' % it])))
    ens.check_flag()
    e = [cuda(d['eps%d' % i]) for i in range(6)]
    elbo = model.elbo(step=0, armortized_bs=bs, eps=(torch.cat([e[0], e[1], e[3]]), torch.cat([e[2], e[4]]), e[5]))
    (-elbo).backward()
    engine = model._elbo_engine(bs, Ns, False, N_vo=Nvo, vo_holdoff=False)
    assert engine.rom.y_weight == model.label_weights().data_ptr() and engine.rom.n == Ns
    assert engine.rom_vo.y_weight is None and engine.rom_vo.yw_stride == 0 and engine.rom_vo.n == Nvo
    val_o, gr_o = P.oracle_partial_vo_fixture_elbo(d, ens.mean.cpu().numpy(), ens.vars.cpu().numpy(), w,
                                                   masks=engine_relu_masks(engine))
    e_o = abs(elbo.item() - val_o) / abs(val_o)
    print('vo + masked supervised: elbo %.6f restatement %.6f (%.2e)' % (elbo.item(), val_o, e_o))
    assert e_o <= 1e-5
    print(check_grads({k: tensor_rel(g, gr_o[k]) for k, g in grads_of(model).items()}, tol_all=5e-5, frac_tight=1.0))
    gls, ref = model.g.logsigmas_y.grad.cpu().numpy(), gr_o['g.logsigmas_y']
    assert np.all(gls[w == 0] != 0)
    assert tensor_rel(gls[w == 0], ref[w == 0]) < 5e-5
