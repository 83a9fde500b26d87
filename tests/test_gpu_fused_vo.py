"""The virtual-observable term in the fused training step (gpi.train.FusedElboStep with X_vo): the
GPI_DRAW_GAUSS item of gpi_draws, the step against the module path (GenerativeModel.elbo + backward) on
the step's own subset and noise, its captured forms, the VO update between replays and the hold-off
switch.  Shapes of vo_elbo_c32.npz / vo_elbo_lockx_c32.npz (32^2 images, [1, 1] blocks).

The module-path reference of every comparison is a second model built from the same fixture (the twin of
a deep copy: same state dict, same VO queries, the same two injected-noise VO updates); the parameters
are copied across before every compared step as test_fused_step_matches_module_path does."""
import functools
import math

import numpy as np
import pytest
import torch

from test_gpu_vo import build_vo_model, load, cuda

pytestmark = pytest.mark.gpu

FIX = {False: 'vo_elbo_c32.npz', True: 'vo_elbo_lockx_c32.npz'}


@functools.lru_cache(maxsize=None)
def fixture(lockx):
    return load(FIX[lockx])


def upd_eps(d, it):
    return cuda(d['upd%d.eps_X' % it]), cuda(d['upd%d.eps_y' % it])


def vo_model(lockx, updates=2):
    """Fixture model with its VO posterior brought into existence as _vo_model_parity does."""
    d = fixture(lockx)
    model, ens, bs = build_vo_model(d, independent_X=not lockx)
    for it in range(updates):
        model.update_virtual_observables(int(d['cfg'][7]), step=it, eps=upd_eps(d, it))
    return d, model, ens, bs


def make_step(d, model, bs, **kw):
    from gpi.train import FusedElboStep
    kw.setdefault('lr', 1e-3)
    kw.setdefault('seed', 7)
    return FusedElboStep(model, cuda(d['Xu']), bs, cuda(d['Xs']), cuda(d['Ys']), cuda(d['Fs']),
                         X_vo=cuda(d['Xv']), F_vo=cuda(d['Fv']), **kw)


def bn_buffers(model):
    return {k: v for k, v in model.state_dict().items()
            if k.endswith(('running_mean', 'running_var', 'num_batches_tracked'))}


def training_state(step, model):
    return [step.flat.P, step.m, step.v, step.step_ctr, step.rng_off, step.lr] + list(bn_buffers(model).values())


def one_round(step, model, ref_model, ens, d, bs, lockx, holdoff, it, y_draw):
    """One forward_backward() / update() round against ref_model.elbo + backward on the step's subset and
    noise.  y_draw = (Philox offset, sub id) the step's pending y_vo was drawn with: eps_y is regenerated
    bit-exactly from it (zero mean, zero logsigma: fmaf(1, z, 0) = z).  Bars of
    test_fused_step_matches_module_path: ELBO 1e-5 relative, every gradient tensor within 1e-4 of its max,
    BN running buffers rtol 1e-5 / atol 1e-6; per-term values 1e-5 relative."""
    from gpi import vo as gvo
    Ns, Nvo = int(d['cfg'][5]), int(d['cfg'][6])
    with torch.no_grad():
        for (k, p), (k2, q) in zip(model.named_parameters(), ref_model.named_parameters()):
            assert k == k2
            q.copy_(p)
        src = bn_buffers(model)             # (the reference may not have taken the step's earlier steps)
        for k, v in bn_buffers(ref_model).items():
            v.copy_(src[k])
    e = step.engine
    assert e.vo_holdoff == holdoff and e.lockx == lockx and e.N_vo == Nvo
    assert e.eps_z().shape[0] == bs + Ns + Nvo
    assert e.N_ex == (0 if lockx else Ns + (0 if holdoff else Nvo))
    eps = [e.eps_z().clone(), None if lockx else e.eps_x().clone()]
    if not holdoff:
        off, sub = y_draw
        zero = torch.zeros_like(ens.mean)
        eps_y = gvo.gauss_sample(torch.empty_like(zero), zero, zero, seed=step.seed, offset=off, sub=sub)
        want = gvo.gauss_sample(torch.empty_like(zero), ens.mean.contiguous(), ens.logsigma.contiguous(),
                                seed=step.seed, offset=off, sub=sub)
        assert torch.equal(e.y_vo(), want), it
        eps.append(eps_y)
    ref_model._datasets['unsupervised'].perm = step.idx.clone().long()
    ref_model.zero_grad()
    ref = ref_model.elbo(step=it, armortized_bs=bs, vo_holdoff=holdoff, eps=tuple(eps))
    ref_terms = ref_model._elbo_engine(bs, Ns, False, N_vo=Nvo, vo_holdoff=holdoff).terms()
    (-ref).backward()
    step.forward_backward()
    torch.cuda.synchronize()
    got, terms = step.elbo().item(), step.terms()
    print('round', it, 'elbo', got, ref.item(), {k: (terms[k], ref_terms[k]) for k in terms if k.startswith('vo_')})
    assert abs(got - ref.item()) <= 1e-5 * abs(ref.item()), (it, got, ref.item())
    keys = ['vo_logL_x', 'vo_DKL'] + ([] if holdoff else ['vo_logL_y'] + ([] if lockx else ['vo_logL_X', 'vo_entropy']))
    assert set(k for k in terms if k.startswith('vo_')) == set(keys)
    for k in keys:
        assert abs(terms[k] - ref_terms[k]) <= 1e-5 * abs(ref_terms[k]), (it, k, terms[k], ref_terms[k])
    G = step.flat.G
    for k, p in ref_model.named_parameters():
        g = G[step.flat.name_offsets[k]:step.flat.name_offsets[k] + p.numel()].view(p.shape)
        ref_g = p.grad if p.grad is not None else torch.zeros_like(p)
        err = (g - ref_g).abs().max().item() / max(ref_g.abs().max().item(), 1.0)
        assert err < 1e-4, (it, k, err)
    if holdoff and not lockx:            # parameters the held-off term does not reach
        qx = model.q_X['vo']
        for p in (qx._mean, qx._logsigma):
            o = step.flat.offset(p)
            assert torch.count_nonzero(G[o:o + p.numel()]).item() == 0
    step.update()
    torch.cuda.synchronize()
    sd, rsd = bn_buffers(model), bn_buffers(ref_model)
    assert sd
    for k in sd:
        torch.testing.assert_close(sd[k], rsd[k], rtol=1e-5, atol=1e-6)


# ---------------------------------------------------------------- 1. the draw kind
def test_draw_gauss_item_matches_gauss_sample(device):
    """One gpi_draws call with a GPI_DRAW_RANDN item and two GPI_DRAW_GAUSS items (n = 3 * 1023 and n = 5:
    no multiples of 4 or 256, so the tail lanes and the block-range split are exercised) at a non-zero
    device offset = gpi_randn / gpi_gauss_sample(rep = 1, eps = NULL) one by one, bit for bit; memory past
    each out keeps its sentinel."""
    from gpi import _lib as L
    from gpi import vo as gvo
    lib, st = L.lib(), L.stream_handle()
    o = torch.tensor([(1 << 33) + 5], dtype=torch.int64, device='cuda')
    seed, pad = 97531, 300
    nr, n1, n2 = 1003, 3 * 1023, 5
    g = torch.Generator(device='cuda').manual_seed(1)
    mean = {n: torch.randn(n, device='cuda', generator=g) for n in (n1, n2)}
    ls = {n: 0.5 * torch.randn(n, device='cuda', generator=g) - 1.0 for n in (n1, n2)}
    a = {n: torch.full((n + pad,), 7.0, device='cuda') for n in (nr, n1, n2)}
    b = {n: v.clone() for n, v in a.items()}
    assert L.GPI_MAX_DRAWS == 6
    items = [L.DrawItem(kind=L.DRAW_RANDN, out=a[nr].data_ptr(), n=nr, sub=2, seed=seed)] + \
        [L.DrawItem(kind=L.DRAW_GAUSS, out=a[n].data_ptr(), n=n, sub=s, seed=seed, mean=mean[n].data_ptr(),
                    logsigma=ls[n].data_ptr()) for n, s in ((n1, 6), (n2, 206))]
    arr = (L.DrawItem * len(items))(*items)
    L.check(lib.gpi_draws(arr, len(items), L.ptr(o), st), 'draws')
    L.check(lib.gpi_randn(L.ptr(b[nr]), nr, seed, L.ptr(o), 2, st), 'randn')
    gvo.gauss_sample(b[n1][:n1].view(3, 1023), mean[n1].view(3, 1023), ls[n1].view(3, 1023), seed=seed, offset=o, sub=6)
    gvo.gauss_sample(b[n2][:n2].view(1, 5), mean[n2].view(1, 5), ls[n2].view(1, 5), seed=seed, offset=o, sub=206)
    torch.cuda.synchronize()
    for n in a:
        assert torch.equal(a[n], b[n]), n
        assert torch.all(a[n][n:] == 7.0) and not torch.any(a[n][:n] == 7.0), n
    z = (a[n1][:n1] - mean[n1]) / torch.exp(ls[n1])          # the normals behind the larger item: N(0, 1)-like
    assert abs(z.mean().item()) < 0.1 and abs(z.std().item() - 1.0) < 0.1
    # a Gauss item without its sources is an argument error, not a launch
    bad = (L.DrawItem * 1)(L.DrawItem(kind=L.DRAW_GAUSS, out=a[n2].data_ptr(), n=n2, sub=1, seed=seed))
    assert lib.gpi_draws(bad, 1, L.ptr(o), st) != 0


# ---------------------------------------------------------------- 2. / 3. the step vs the module path
@pytest.mark.parametrize('holdoff', [False, True], ids=['active', 'holdoff'])
@pytest.mark.parametrize('lockx', [False, True], ids=['freeX', 'lockX'])
def test_fused_vo_step_matches_module_path(device, lockx, holdoff):
    """Two forward_backward() / update() rounds of the step with the VO term (and its hold-off variant)
    against the module path on the step's own subset and noise; see one_round.  The first round's y_vo is
    the constructor's draw (sub 106), the second's was drawn during the first round's backward (sub 6),
    both at the Philox offset of the time of the draw."""
    from gpi.train import VO_Y_SUB
    d, model, ens, bs = vo_model(lockx)
    _, ref_model, _, _ = vo_model(lockx)
    step = make_step(d, model, bs, vo_holdoff=holdoff)
    assert step.rng_span >= int(d['cfg'][6]) * step.engine.d_y
    y_draw = (step.rng_off.clone(), 100 + VO_Y_SUB)
    for it in range(2):
        off = step.rng_off.clone()
        one_round(step, model, ref_model, ens, d, bs, lockx, holdoff, it, y_draw)
        y_draw = (off, VO_Y_SUB)
    assert step.step_ctr.item() == 2
    step.check_handoff()
    step.engine.check_flag()


def test_multi_launch_draws_match_one_launch(device, monkeypatch):
    """GPI_ONE_DRAW=0 (the multi-launch fallback, also taken by pools above 16384) draws the same y_vo, eps_z
    and eps_X as the one-launch form: same seed / offset / sub."""
    d, model, ens, bs = vo_model(False)
    a = make_step(d, model, bs)
    monkeypatch.setenv('GPI_ONE_DRAW', '0')
    d2, model2, _, _ = vo_model(False)
    b = make_step(d2, model2, bs)
    assert a._one_draw and not b._one_draw
    for _ in range(2):
        torch.cuda.synchronize()
        for x, y in ((a.engine.y_vo(), b.engine.y_vo()), (a.engine.eps_z(), b.engine.eps_z()),
                     (a.engine.eps_x(), b.engine.eps_x()), (a.idx, b.idx)):
            assert torch.equal(x, y)
        a.step()
        b.step()
    torch.cuda.synchronize()
    assert torch.equal(a.flat.P, b.flat.P)


# ---------------------------------------------------------------- 4. capture
@pytest.mark.parametrize('mode', ['single', 'streams', 'segments'])
def test_captured_vo_step_matches_eager(device, mode, monkeypatch):
    """A captured step with the VO term against an eager twin over four steps, with a VO update (same
    injected noise on both) after the second: capture() leaves every buffer a step writes bit-identical,
    ELBO within 1e-6 relative, parameters rtol 1e-6 / atol 1e-7, no hand-off timed out."""
    d, model_a, _, bs = vo_model(False)
    _, model_b, _, _ = vo_model(False)
    eager = make_step(d, model_a, bs, seed=3)
    monkeypatch.setenv('GPI_GRAPH_MODE', mode)
    graph = make_step(d, model_b, bs, seed=3)
    monkeypatch.delenv('GPI_GRAPH_MODE')
    # ('streams' falls back to 'single' when the probe finds the two streams on one hardware queue)
    assert graph.graph_mode == mode or (mode == 'streams' and graph.graph_mode == 'single')
    mode = graph.graph_mode
    before = [t.clone() for t in graph._mutable_state()]
    graph.capture()
    torch.cuda.synchronize()
    for t, b in zip(graph._mutable_state(), before):
        assert torch.equal(t, b)
    for n in range(4):
        if n == 2:
            for s in (eager, graph):
                s.update_virtual_observables(int(d['cfg'][7]), step=2, eps=upd_eps(d, 1))
            assert torch.equal(eager.engine.y_vo(), graph.engine.y_vo())
        eager.step()
        graph.step()
        torch.cuda.synchronize()
        assert abs(eager.elbo().item() - graph.elbo().item()) <= 1e-6 * abs(eager.elbo().item())
        torch.testing.assert_close(graph.flat.P, eager.flat.P, rtol=1e-6, atol=1e-7)
        assert math.isfinite(graph.terms()['vo_logL_y'])
    assert graph.step_ctr.item() == eager.step_ctr.item() == 4
    assert graph.graph is not None
    assert (graph.segs is not None) == (mode == 'segments')
    assert (graph.g_side is not None) == (mode == 'streams')
    graph.check_handoff()
    eager.check_handoff()


def test_unrolled_vo_graph_matches_single_steps(device):
    """capture(unroll=2) + run(4) leaves exactly the parameters and Adam moments that four step() replays
    leave (test_unrolled_graph_matches_single_steps' standard), with the second ROM launch and the y_vo
    draw in the unrolled pair.  (On a shared hardware queue the step falls back to 'single' and run()
    replays single steps: the comparison holds there too.)"""
    d, model_a, _, bs = vo_model(False)
    _, model_b, _, _ = vo_model(False)
    one = make_step(d, model_a, bs, seed=3)
    unr = make_step(d, model_b, bs, seed=3)
    one.capture()
    unr.capture(unroll=2)
    assert unr.unroll == (2 if unr.graph_mode == 'streams' else 1)
    for _ in range(4):
        one.step()
    unr.run(4)
    torch.cuda.synchronize()
    unr.check_handoff()
    for a, b in ((one.flat.P, unr.flat.P), (one.m, unr.m), (one.v, unr.v), (one.step_ctr, unr.step_ctr),
                 (one.engine.y_vo(), unr.engine.y_vo())):
        assert torch.equal(a, b)
    assert int(unr.step_ctr.item()) == 4


def test_early_rom_with_vo_matches_default_order(device, monkeypatch):
    """GPI_ROM_EARLY=1 with the VO term: both ROM launches draw their X~ rows in the kernel at the start of
    the step; bit for bit what the default order leaves over three replays (where the stream pair shares a
    hardware queue there is no side step gate and the ROMs stay after the head forward: same result)."""
    d, model_a, _, bs = vo_model(False)
    _, model_b, _, _ = vo_model(False)
    late = make_step(d, model_a, bs, seed=3)
    monkeypatch.setenv('GPI_ROM_EARLY', '1')
    early = make_step(d, model_b, bs, seed=3)
    assert early.engine.rom_draw and not late.engine.rom_draw
    late.capture()
    early.capture()
    assert early.engine.rom_early_launched == (early.graph_mode == 'streams')
    for _ in range(3):
        late.step()
        early.step()
    torch.cuda.synchronize()
    early.check_handoff()
    for a, b in ((late.flat.P, early.flat.P), (late.m, early.m), (late.v, early.v),
                 (late.last_terms, early.last_terms)):
        assert torch.equal(a, b)


# ---------------------------------------------------------------- 5. the update refreshes the pending target
def test_vo_update_redraws_pending_target(device):
    from gpi import vo as gvo
    from gpi.train import VO_REDRAW_SUB, vo_buffers
    d, model, ens, bs = vo_model(False)
    step = make_step(d, model, bs)
    step.step()                                   # (parameters move: the third update sees another q_X['vo'])
    torch.cuda.synchronize()
    ptrs = [t.data_ptr() for t in vo_buffers(ens)]
    y0, mean0 = step.engine.y_vo().clone(), ens.mean.clone()
    off = step.rng_off.clone()
    step.update_virtual_observables(int(d['cfg'][7]), step=2, eps=upd_eps(d, 1))
    assert not torch.equal(ens.mean, mean0)
    assert not torch.equal(step.engine.y_vo(), y0)
    want = gvo.gauss_sample(torch.empty_like(y0), ens.mean.contiguous(), ens.logsigma.contiguous(), seed=step.seed,
                            offset=off, sub=VO_REDRAW_SUB)
    assert torch.equal(step.engine.y_vo(), want)
    assert [t.data_ptr() for t in vo_buffers(ens)] == ptrs
    assert torch.equal(step.rng_off, off)
    ens.check_flag()
    step.forward_backward()
    with pytest.raises(RuntimeError, match='between forward_backward'):
        step.update_virtual_observables(int(d['cfg'][7]), step=3, eps=upd_eps(d, 1))
    with pytest.raises(RuntimeError, match='between forward_backward'):
        step.set_vo_holdoff(True)
    step.update()
    torch.cuda.synchronize()
    assert step.step_ctr.item() == 2


def test_fused_vo_step_energy_ensemble(device):
    """The other ensemble family (EnergyVirtualObservablesEnsemble, its _EnergyState.mean32 / logsig32
    buffers): the constructor's target, a captured step, the update's redraw from the buffers the energy
    kernel wrote in place, and a step after it."""
    from gpi import vo as gvo
    from gpi.train import VO_REDRAW_SUB, VO_Y_SUB, vo_buffers
    from test_gpu_energy_vo import build_energy_vo_model
    d = load('vo_energy_elbo_c32.npz')
    model, ens, bs = build_energy_vo_model(d)
    for it in range(2):
        model.update_virtual_observables(int(d['cfg'][7]), step=it, eps=upd_eps(d, it))
    step = make_step(d, model, bs)
    assert step.vo is ens and vo_buffers(ens)[0] is ens._state.mean32
    ptrs = [t.data_ptr() for t in vo_buffers(ens)]

    def target(off, sub):
        return gvo.gauss_sample(torch.empty_like(step.engine.y_vo()), ens.mean.contiguous(), ens.logsigma.contiguous(),
                                seed=step.seed, offset=off, sub=sub)

    assert torch.equal(step.engine.y_vo(), target(step.rng_off.clone(), 100 + VO_Y_SUB))
    step.capture()
    off = step.rng_off.clone()
    step.step()
    torch.cuda.synchronize()
    assert torch.equal(step.engine.y_vo(), target(off, VO_Y_SUB))         # drawn during that step, for the next
    off, mean0 = step.rng_off.clone(), ens.mean.clone()
    step.update_virtual_observables(int(d['cfg'][7]), step=2, eps=upd_eps(d, 1))
    assert not torch.equal(ens.mean, mean0)
    assert torch.equal(step.engine.y_vo(), target(off, VO_REDRAW_SUB))
    assert [t.data_ptr() for t in vo_buffers(ens)] == ptrs
    step.step()
    torch.cuda.synchronize()
    assert math.isfinite(step.elbo().item()) and all(math.isfinite(v) for v in step.terms().values())
    assert step.step_ctr.item() == 2
    ens.check_flag()
    step.engine.check_flag()
    step.check_handoff()


# ---------------------------------------------------------------- 6. the hold-off switch
def test_vo_holdoff_switch(device):
    """Two held-off (captured) steps, set_vo_holdoff(False): parameters, Adam moments, step counter, Philox
    offset, learning rate and BN running buffers bit-identical across the switch, the graphs dropped, and
    the next step the module path's elbo(vo_holdoff=False) on the same noise (bars of one_round; its y_vo
    from sub VO_SWITCH_SUB0 + 6 at the current offset).  Switching back: the same."""
    from gpi.train import VO_SWITCH_SUB0, VO_Y_SUB
    lockx = False
    d, model, ens, bs = vo_model(lockx)
    _, ref_model, _, _ = vo_model(lockx)
    step = make_step(d, model, bs, vo_holdoff=True)
    step.capture()
    for _ in range(2):
        step.step()
    torch.cuda.synchronize()
    sched = step.optimizer
    for it, flag in enumerate((False, True)):
        before = [t.clone() for t in training_state(step, model)]
        idx = step.idx.clone()
        step.set_vo_holdoff(flag)
        torch.cuda.synchronize()
        for t, b in zip(training_state(step, model), before):
            assert torch.equal(t, b)
        assert torch.equal(step.idx, idx) and step.optimizer is sched
        assert step.graph is None and step.engine.vo_holdoff == flag
        one_round(step, model, ref_model, ens, d, bs, lockx, flag, it, (step.rng_off.clone(), VO_SWITCH_SUB0 + VO_Y_SUB))
    assert step.step_ctr.item() == 4
    step.capture()                               # replays again after a new capture
    step.step()
    torch.cuda.synchronize()
    assert step.step_ctr.item() == 5 and math.isfinite(step.elbo().item())
    step.check_handoff()


# ---------------------------------------------------------------- 7. refusals
def test_fused_vo_refusals(device):
    from gpi import _lib as L
    d = fixture(False)
    model, ens, bs = build_vo_model(d)
    with pytest.raises(ValueError, match='single process'):
        make_step(d, model, bs, world=2, rank=0, subset_seed=1)
    with pytest.raises(RuntimeError, match='no posterior yet'):
        make_step(d, model, bs)
    held = make_step(d, model, bs, vo_holdoff=True)      # (no target is drawn while the term is held off)
    with pytest.raises(RuntimeError, match='no posterior yet'):
        held.set_vo_holdoff(False)
    assert held.engine.vo_holdoff
    for it in range(2):
        model.update_virtual_observables(int(d['cfg'][7]), step=it, eps=upd_eps(d, it))
    step = make_step(d, model, bs)
    ens._mean32 = ens._mean32.clone()
    with pytest.raises(L.NativeError, match='rebuild the step'):
        step.update_virtual_observables(int(d['cfg'][7]), step=2, eps=upd_eps(d, 1))
    from gpi.train import FusedElboStep
    plain = FusedElboStep(model, cuda(d['Xu']), bs, cuda(d['Xs']), cuda(d['Ys']), cuda(d['Fs']))
    with pytest.raises(L.NativeError, match='without X_vo'):
        plain.update_virtual_observables(4, step=0)


# ---------------------------------------------------------------- 8. loop smoke
def test_fused_vo_loop_smoke(device, tmp_path):
    """The highres32 factories as in test_gpu_training plus 8 VO samples with CGR + flux rows: 40 captured
    steps, held off for the first 10, a VO update at the switch and every 10 steps after.  A smoke, not a
    convergence claim (the objective changes definition at the switch and at every update): every ELBO and
    term finite, the error flags clean, 40 steps counted."""
    from factories.model import ModelFactory
    from factories.data import DataFactory
    from utils.data import DataSet
    from bottleneck import VirtualObservables as VO
    from physics.BoundaryConditions import BoundaryCondition
    from physics.grid import pixel_to_cells
    from gpi.train import FusedElboStep
    from test_gpu_vo import _DS
    torch.manual_seed(1)
    fac = ModelFactory.FromIdentifier('highres32')
    fac.set('device', 'cuda')
    physics, model, _, encoder, dtype, dev = fac.setup()
    df = DataFactory.FromIdentifier('highres32', device=dev, seed=1, path=str(tmp_path) + '/')
    dl, dlu = df.setup()
    dl.assemble(physics, indices=range(16), device=dev)
    sup = DataSet(dl, np.arange(16), device=dev, label='supervised')
    unsup = DataSet(dlu, np.arange(64), device=dev, label='unsupervised')
    n = physics['fom'].grid.n
    rng = np.random.default_rng(3)
    N_vo = 8
    X = rng.normal(0.4, 0.8, (N_vo, n, n))
    U = rng.uniform(-0.5, 0.5, (N_vo, 4))
    F = np.stack([physics['rom'].grid.full_force(u) for u in U])
    QPE = VO.QuerryPointEnsemble([VO.QuerryPoint(physics['fom'], pixel_to_cells(x), BoundaryCondition(u))
                                  for x, u in zip(X, U)])
    QE = VO.QuerryEnsemble.FromQuerryPointEnsemble(QPE, physics, True, True, 0, 0, dtype=torch.float32, device=dev)
    ens = VO.VirtualObservablesEnsemble(QPE, QE, dtype=torch.float32, device=dev)
    vo_ds = _DS(X=cuda(X), Y=cuda(np.zeros((N_vo, (n + 1) * (n - 1)))), F_ROM_BC=cuda(F))
    model.encoder = encoder
    model.register_datasets({'supervised': sup, 'unsupervised': unsup, 'vo': vo_ds}, ens,
                            create_unsupervised_variational_approximation=False)
    step = FusedElboStep(model, unsup.get('X'), 32, sup.get('X'), sup.get('Y'), sup.get('F_ROM_BC'), lr=1e-2, seed=3,
                         X_vo=vo_ds.get('X'), F_vo=vo_ds.get('F_ROM_BC'), vo_holdoff=True)
    step.capture()
    elbos, terms = [], []
    for it in range(40):
        if it >= 10 and it % 10 == 0:
            step.update_virtual_observables(16, step=it)
            if it == 10:
                step.set_vo_holdoff(False)
                step.capture()
        step.step()
        elbos.append(step.elbo())
        terms.append(step.terms())
    torch.cuda.synchronize()
    assert all(math.isfinite(float(e.item())) for e in elbos)
    assert all(math.isfinite(v) for t in terms for v in t.values())
    assert 'vo_logL_y' not in terms[9] and 'vo_logL_y' in terms[10] and 'vo_DKL' in terms[0]
    step.engine.check_flag()
    ens.check_flag()
    step.check_handoff()
    assert step.step_ctr.item() == 40
