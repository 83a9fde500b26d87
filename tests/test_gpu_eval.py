"""GPU: the eval-mode (inference) path -- running-statistic BatchNorm codec engines, the surrogate
predictor and its graph capture -- against the fp64 eval restatement (tests/eval_ref.py, 1e-5 relative
norm: the project's fp32 criterion) and the reference's own eval-mode run (codec_eval_*.npz, 1e-4 of the
tensor's max as the other codec tests use)."""
import copy
import os

import numpy as np
import pytest
import torch

import eval_ref
from eval_ref import relnorm

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), 'golden')
TOL = 1e-5


def load(name):
    return dict(np.load(os.path.join(GOLD, name), allow_pickle=False))


def cuda(a, dtype=torch.float32):
    return torch.tensor(np.asarray(a), dtype=dtype, device='cuda')


def rel(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


_CASES = {}


def case(tag):
    """(fixture, restatement outputs) of one configuration, computed once for all tests."""
    if tag not in _CASES:
        d = load('codec_eval_%s.npz' % tag)
        _CASES[tag] = (d, eval_ref.fixture_eval(d))
    return _CASES[tag]


def modules(d, which=('enc', 'dec')):
    from bottleneck.Encoder import CNNEncoder
    from bottleneck.Decoder import CNNDecoder
    imsize, dz, latent, growth, f_enc, f_dec, blocks = eval_ref.fixture_cfg(d)
    p = float(d['p'])
    out = []
    if 'enc' in which:
        enc = CNNEncoder(imsize, dz, blocks, growth, f_enc, drop_rate=p)
        enc.load_state_dict({k[4:]: torch.tensor(v) for k, v in d.items() if k.startswith('enc.')})
        out.append(enc.cuda())
    if 'dec' in which:
        dec = CNNDecoder(imsize, dz, (latent, latent), 1, f_dec, blocks, False, growth, drop_rate=p)
        dec.load_state_dict({k[4:]: torch.tensor(v) for k, v in d.items() if k.startswith('dec.')})
        out.append(dec.cuda())
    return out


def buffers(module):
    return {k: v.clone() for k, v in module.state_dict().items() if 'running_' in k or 'num_batches' in k}


# ---------------------------------------------------------------- 1. parity
@pytest.mark.parametrize('tag', ['c32', 'c64'])
def test_eval_codec_matches_restatement_and_reference(device, tag):
    d, ref = case(tag)
    enc, dec = modules(d)
    enc.eval()
    dec.eval()
    mu, ls = enc(cuda(d['X']))
    mx, lsx = dec(cuda(d['Z']))
    assert not mu.requires_grad and not mx.requires_grad
    got = dict(enc_mu=mu, enc_ls=ls, dec_mu=mx, dec_ls=lsx)
    errs = {k: (relnorm(v.cpu(), ref[k]), rel(v.cpu(), d[k])) for k, v in got.items()}
    print(tag, {k: '%.2e / %.2e' % e for k, e in errs.items()})
    for k, (e_ref, e_fix) in errs.items():
        assert got[k].shape == d[k].shape
        assert e_ref < TOL, (k, e_ref)
        assert e_fix < 1e-4, (k, e_fix)


# ---------------------------------------------------------------- 2. determinism
def test_eval_is_deterministic_and_leaves_the_buffers_alone(device):
    d, _ = case('c32')
    enc, dec = modules(d)
    enc.eval()
    dec.eval()
    assert enc._cfg['drop_rate'] == 0.2 and dec._cfg['drop_rate'] == 0.2
    be, bd = buffers(enc), buffers(dec)
    X, Z = cuda(d['X']), cuda(d['Z'])
    a, b = enc(X), enc(X)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    u, v = dec(Z), dec(Z)
    assert torch.equal(u[0], v[0]) and torch.equal(u[1], v[1])
    for before, m in ((be, enc), (bd, dec)):
        after = buffers(m)
        assert len(before) > 0 and all(torch.equal(before[k], after[k]) for k in before)


# ---------------------------------------------------------------- 3. batch independence
@pytest.mark.parametrize('tag', ['c32', 'c64'])
def test_eval_prediction_does_not_depend_on_batch_mates(device, tag):
    d, ref = case(tag)
    enc, dec = modules(d)
    enc.eval()
    dec.eval()
    X, Z = cuda(d['X']), cuda(d['Z'])
    full = enc(X) + dec(Z)
    one = enc(X[:1]) + dec(Z[:1])
    keys = ('enc_mu', 'enc_ls', 'dec_mu', 'dec_ls')
    imsize, dz, latent, growth, f_enc, f_dec, blocks = eval_ref.fixture_cfg(d)
    r1 = eval_ref.encoder_eval(eval_ref.state64(d, 'enc.'), d['X'][:1], imsize, blocks, growth, f_enc) + \
        eval_ref.decoder_eval(eval_ref.state64(d, 'dec.'), d['Z'][:1], latent, blocks, growth, f_dec)
    for k, f, o, r in zip(keys, full, one, r1):
        e_row, e_ref = relnorm(f[:1].cpu(), o.cpu()), relnorm(o.cpu(), r.numpy())
        print(tag, k, 'row 0 of B=3 vs B=1 %.2e, B=1 vs restatement %.2e' % (e_row, e_ref))
        assert e_row < TOL, (k, e_row)
        assert e_ref < TOL, (k, e_ref)
        assert relnorm(r.numpy(), ref[k][:1]) < 1e-12          # the restatement itself is per-sample


# ---------------------------------------------------------------- 4. train path unharmed
@pytest.mark.parametrize('which', ['enc', 'dec'])
def test_train_mode_after_eval_is_bit_identical_and_feeds_the_next_eval(device, which):
    d, _ = case('c32')
    imsize, dz, latent, growth, f_enc, f_dec, blocks = eval_ref.fixture_cfg(d)
    inp = cuda(d['X'] if which == 'enc' else d['Z'])
    fresh, = modules(d, (which,))
    torch.manual_seed(5)                       # the Dropout2d draws take their Philox seed from torch's generator
    want = fresh(inp)
    m, = modules(d, (which,))
    m.eval()
    before = buffers(m)
    m(inp)
    m.train()
    torch.manual_seed(5)
    got = m(inp)
    assert all(torch.equal(a.detach(), b.detach()) for a, b in zip(got, want))
    assert got[0].requires_grad
    after = buffers(m)
    assert all(torch.equal(after[k], buffers(fresh)[k]) for k in after)
    assert any(not torch.equal(before[k], after[k]) for k in before)
    m.eval()
    out = m(inp)
    st = eval_ref.state64({k: v for k, v in m.state_dict().items()}, '')
    if which == 'enc':
        r = eval_ref.encoder_eval(st, d['X'], imsize, blocks, growth, f_enc)
    else:
        r = eval_ref.decoder_eval(st, d['Z'], latent, blocks, growth, f_dec)
    for o, rr in zip(out, r):
        e = relnorm(o.cpu(), rr.numpy())
        print(which, 'eval after a train step: %.2e' % e)
        assert e < TOL, e


# ---------------------------------------------------------------- 5. / 6. surrogate
def _surrogate():
    """DiscriminativeModel extracted from the elbo_c32 golden model after loading a state with
    randomised (per BN layer) running buffers; its fp64 reference composition."""
    from test_gpu_parity import build_golden_model
    from oracle import elbo as oelbo
    d = load('elbo_c32.npz')
    model, _ = build_golden_model(d)
    gen = torch.Generator().manual_seed(17)
    st = model.encoder.state_dict()
    for k, v in st.items():
        if k.endswith('running_mean'):
            st[k] = (0.5 * torch.randn(v.shape, generator=gen)).cuda()
        elif k.endswith('running_var'):
            st[k] = (0.5 + torch.rand(v.shape, generator=gen)).cuda()
    model.encoder.load_state_dict(st)
    # the encoder has native caches (flat buffer, an engine) by the time it is deep-copied
    model.encoder.eval()
    model.encoder(cuda(d['Xs']))
    disc = model.extract_discriminative_model(FromLatentEncoding=False, duplicate=True)
    disc.eval()
    n, nc, dz = [int(v) for v in d['cfg'][:3]]
    t = lambda k: torch.tensor(d[k], dtype=torch.float64)
    es = eval_ref.state64(dict(disc._encoder.state_dict()), '')
    w, b = disc._gp.weight.detach().double().cpu(), disc._gp.bias.detach().double().cpu()
    lsy = disc._g.logsigmas_y.detach().double().cpu()
    bc = torch.as_tensor(d['bc_dofs'])

    def reference(X):
        mu, ls = eval_ref.encoder_eval(es, X, n, [1, 1], 4, 4)
        return mu, ls, (lambda z, F: oelbo.rom_operator(t('W'), t('M'), bc, z @ w.t() + b, F, lsy)[0])

    return d, model, disc, reference, (w, b, lsy, t('W'), t('M'), bc)


def test_discriminative_model_eval_forward_and_mc(device):
    from oracle import elbo as oelbo
    d, model, disc, reference, (w, b, lsy, W, M, bc) = _surrogate()
    # the deepcopy in extract_discriminative_model shares no native cache with the model's encoder
    assert not any(k.startswith('_gpi_') for m in disc._encoder.modules() for k in m.__dict__)
    X, F = cuda(d['Xs']), cuda(d['F'])
    y, ls_y = disc(X, F)
    assert not y.requires_grad and ls_y.shape == y.shape
    y2, _ = disc(X, F)
    assert torch.equal(y, y2)
    assert disc._encoder._gpi_flat is not getattr(model.encoder, '_gpi_flat', None)
    mu, ls, rom = reference(d['Xs'])
    F64 = torch.tensor(d['F'], dtype=torch.float64)
    want = rom(mu, F64)
    e = relnorm(y.cpu(), want.numpy())
    print('DiscriminativeModel eval forward vs fp64 composition: %.2e' % e)
    assert e < TOL, e
    disc.predictor(X.shape[0]).check_flag()
    # MC predictive with injected noise
    N, N_mc = X.shape[0], 8
    gen = torch.Generator().manual_seed(3)
    eps_z = torch.randn(N * N_mc, mu.shape[1], generator=gen)
    eps_y = torch.randn(N * N_mc, want.shape[1], generator=gen)
    mean, std = disc.predict_mc(X, F, N_mc, eps=(eps_z.cuda(), None, eps_y.cuda()))
    m_o, s_o = oelbo.vo_predictive(W, M, bc, mu, ls, F64, lsy, eps_z.double().reshape(N, N_mc, -1),
                                   eps_y.double().reshape(N, N_mc, -1), gp_linear=lambda z: z @ w.t() + b)
    em, es_ = rel(mean.cpu(), m_o.numpy()), rel(std.cpu(), s_o.numpy())
    print('predict_mc mean %.2e std %.2e' % (em, es_))
    assert em < 1e-4 and es_ < 1e-4
    # train mode keeps the differentiable module path (and its return type)
    disc.train()
    yt, lst = disc(X, F)
    assert yt.shape == y.shape and lst.shape == ls_y.shape


def test_surrogate_predictor_capture(device):
    from gpi.infer import SurrogatePredictor
    d, model, disc, reference, _ = _surrogate()
    X, F = cuda(d['Xs']), cuda(d['F'])
    p = SurrogatePredictor(disc, X.shape[0])
    y0 = p.predict(X, F).clone()
    p.capture()
    y1 = p.replay().clone()
    assert torch.equal(y0, y1)
    X2 = torch.roll(X, 1, 0).contiguous()
    p.X.copy_(X2.reshape(p.X.shape))
    y2 = p.replay().clone()
    y2u = p.predict().clone()
    assert torch.equal(y2, y2u)
    assert not torch.equal(y2, y0)
    F64 = torch.tensor(d['F'], dtype=torch.float64)
    mu, _, rom = reference(np.roll(d['Xs'], 1, 0))
    assert relnorm(y2.cpu(), rom(mu, F64).numpy()) < TOL
    # a predictor built from the GenerativeModel and its encoder gives the same prediction
    q = SurrogatePredictor(model, X.shape[0])
    assert torch.equal(q.predict(X, F), y0)
    p.check_flag()


# ---------------------------------------------------------------- 7. the ELBO ignores .eval()
def test_elbo_ignores_eval_mode(device):
    from test_gpu_parity import build_golden_model
    d = load('elbo_c32.npz')
    model, bs = build_golden_model(d)
    eps = (torch.cat([cuda(d['eps_enc']), cuda(d['eps_qz'])]), cuda(d['eps_qX']))

    def run():
        for p in model.parameters():
            p.grad = None
        elbo = model.elbo(step=0, armortized_bs=bs, eps=eps)
        (-elbo).backward()
        return elbo.item(), {k: p.grad.clone() for k, p in model.named_parameters()}

    # (same = to 1e-6: the fp64 accumulators take their atomic adds in a varying order, so two runs of
    # one mode differ in the last fp32 bit at most; a mode-dependent BN or dropout would differ at O(1))
    v0, g0 = run()
    model.eval()
    assert not model.encoder.training and not model.f.training
    v1, g1 = run()
    assert abs(v1 - v0) <= 1e-6 * abs(v0), (v0, v1)
    assert abs(v0 - float(d['elbo'])) / abs(float(d['elbo'])) < 2e-5
    for k in g0:
        assert rel(g1[k].cpu(), g0[k].cpu()) < 1e-6, k
