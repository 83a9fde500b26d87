"""GPU, operator level: gpi_gpmlp_forward / gpi_gpmlp_backward / gpi_gpmlp_sample (the nonlinear effective-property
map, csrc/gpmlp.hip) against a plain fp64 torch evaluation on seeded inputs.

The loss the backward differentiates is the gp term of -ELBO as the head forms it, with the ROM adjoint standing
in as a fixed cotangent G = gxs on X~:
    free-X:  J = sum_rows  -lx_s (logL_X + sum logsigma_qX)  +  <G, X~>,   X~ = q_X mean + exp(q_X logsigma) eps_x
    lock-X:  J = <G, mu_X>,                                                   X~ = mu_X
with z = q_z mean + exp(q_z logsigma) eps_z, so the q_z rows receive W_1^T delta_1 through z.
Bars: stored mu_X, X~, h_k 1e-5 (max|d| / max|ref| per tensor), terms 1e-5, every gradient tensor 5e-5.
Inputs are drawn row by row until every fp64 hidden pre-activation is >= 1e-3 from zero (asserted on the host before
any launch): no hidden ReLU decision depends on fp32 rounding."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SENT = 12345.0
MARGIN = 1e-3
LOG2PI = math.log(2 * math.pi)


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def mlp64(Ws, bs, z, pre=None):
    h = z
    for k, (w, b) in enumerate(zip(Ws, bs)):
        a = torch.nn.functional.linear(h, w, b)
        if k == len(Ws) - 1:
            return a, h
        if pre is not None:
            pre.append(a)
        h = torch.relu(a)


class Case(object):
    """One seeded problem: widths [d_z, w_1 .. w_L, d_x], segments [(rows, lx_scale)] (one or two)."""

    def __init__(self, widths, segs, lockx, seed=0):
        self.widths, self.segs, self.lockx = list(widths), list(segs), bool(lockx)
        self.L = len(widths) - 2
        self.n = sum(n for n, _ in segs)
        g = torch.Generator().manual_seed(seed)
        rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
        dz, dx = widths[0], widths[-1]
        self.W = [(torch.rand(widths[k + 1], widths[k], generator=g, dtype=torch.float64) * 2 - 1) / math.sqrt(widths[k])
                  for k in range(self.L + 1)]
        self.b = [(torch.rand(widths[k + 1], generator=g, dtype=torch.float64) * 2 - 1) / math.sqrt(widths[k])
                  for k in range(self.L + 1)]
        self.gp_ls = -0.5 + 0.2 * rn(dx)
        # rows of q_z / eps_z redrawn until the row's hidden pre-activations clear the margin
        qz_mu, qz_ls, eps_z = [], [], []
        for _ in range(self.n):
            for attempt in range(200):
                m, s, e = 0.5 * rn(dz), -1.0 + 0.3 * rn(dz), rn(dz)
                pre = []
                mlp64(self.W, self.b, (m + torch.exp(s) * e).float().double()[None], pre)
                if min(float(a.abs().min()) for a in pre) >= 2 * MARGIN:
                    break
            else:
                raise AssertionError('no admissible row found')
            qz_mu.append(m), qz_ls.append(s), eps_z.append(e)
        f32 = lambda t: t.float().double()              # the values the kernels see
        self.qz_mu, self.qz_ls, self.eps_z = f32(torch.stack(qz_mu)), f32(torch.stack(qz_ls)), f32(torch.stack(eps_z))
        self.qx_mu, self.qx_ls, self.eps_x = f32(0.5 * rn(self.n, dx)), f32(-1.0 + 0.3 * rn(self.n, dx)), f32(rn(self.n, dx))
        self.gxs = f32(rn(self.n, dx))
        self.W, self.b, self.gp_ls = [f32(w) for w in self.W], [f32(b) for b in self.b], f32(self.gp_ls)
        self.lx = torch.cat([torch.full((n,), float(np.float32(s)), dtype=torch.float64) for n, s in segs])

    # ---- fp64 reference
    def reference(self):
        leaves = dict(gp_ls=self.gp_ls, qz_mu=self.qz_mu, qz_ls=self.qz_ls, qx_mu=self.qx_mu, qx_ls=self.qx_ls)
        leaves.update({'W%d' % k: w for k, w in enumerate(self.W)})
        leaves.update({'b%d' % k: b for k, b in enumerate(self.b)})
        p = {k: v.clone().requires_grad_() for k, v in leaves.items()}
        # z as the head stores it: fp32 fmaf of fp32 operands (the kernels read it from the workspace)
        z32 = torch.tensor(np.float32(np.float32(self.qz_mu.numpy()) + np.exp(np.float32(self.qz_ls.numpy())).astype(np.float32)
                                      * np.float32(self.eps_z.numpy())))
        z = p['qz_mu'] + torch.exp(p['qz_ls']) * self.eps_z
        z = z + (z32.double() - z).detach()             # the stored value, the exact dependence on the q_z rows
        z.retain_grad()
        pre, hs = [], []
        Ws, bs = [p['W%d' % k] for k in range(self.L + 1)], [p['b%d' % k] for k in range(self.L + 1)]
        mux, _ = mlp64(Ws, bs, z, pre)
        assert min(float(a.detach().abs().min()) for a in pre) >= MARGIN
        hs = [torch.relu(a).detach() for a in pre]
        out = dict(z32=z32, mux=mux.detach(), h=hs)
        if self.lockx:
            out['xs'] = mux.detach()
            J = (self.gxs * mux).sum()
        else:
            xs = p['qx_mu'] + torch.exp(p['qx_ls']) * self.eps_x
            r = xs - mux
            lx_row = (-0.5 * (2 * p['gp_ls'] + r * r * torch.exp(-2 * p['gp_ls']) + LOG2PI)).sum(1)
            ent_row = p['qx_ls'].sum(1)
            out.update(xs=xs.detach(), logL_X=lx_row.detach(), ent=ent_row.detach())
            J = -(self.lx * (lx_row + ent_row)).sum() + (self.gxs * xs).sum()
        J.backward()
        out['grad'] = {k: v.grad for k, v in p.items() if v.grad is not None}
        out['dz'] = z.grad                               # W_1^T delta_1
        return out

    # ---- device layout
    def layout(self, dev):
        from gpi import _lib as Lb
        f = lambda t: t.float()
        n1 = self.segs[0][0]
        P, off = [], {}

        def put(name, t, pad):
            P.append(torch.zeros(pad))                  # odd offsets: no 16-byte alignment anywhere
            off[name] = sum(x.numel() for x in P)
            P.append(f(t).reshape(-1))

        for k in range(self.L + 1):
            put('W%d' % k, self.W[k], 1)
            put('b%d' % k, self.b[k], 2)
        put('gp_ls', self.gp_ls, 1)
        for name, t in (('qz_mu', self.qz_mu), ('qz_ls', self.qz_ls), ('qx_mu', self.qx_mu), ('qx_ls', self.qx_ls)):
            put(name, t[:n1], 3)
            put(name + '2', t[n1:], 1)
        self.P = torch.cat(P).to(dev)
        self.off = off
        wsz, woff = 3, {}

        def alloc(name, numel):
            nonlocal wsz
            woff[name] = wsz
            wsz += numel + 5                            # sentinel gaps between the buffers
        dz, dx = self.widths[0], self.widths[-1]
        for name in ('z', 'eps_z', 'dz'):
            alloc(name, self.n * dz)
        for k in range(1, self.L + 1):
            alloc('h%d' % k, self.n * self.widths[k])
            alloc('dh%d' % k, self.n * self.widths[k])
        for name in ('eps_x', 'xs', 'mux', 'gxs', 'gmux'):
            alloc(name, self.n * dx)
        self.woff, self.wsz = woff, wsz
        ws = torch.full((wsz,), SENT, dtype=torch.float32)
        ref = self.reference()
        for name, t in (('z', ref['z32']), ('eps_z', self.eps_z), ('eps_x', self.eps_x), ('gxs', self.gxs)):
            ws[woff[name]:woff[name] + t.numel()] = f(t).reshape(-1)
        self.ws0 = ws
        self.ref = ref
        R = Lb.GPI_REPLICAS
        self.terms = torch.zeros(4 * R + 2, dtype=torch.float64, device=dev)
        self.terms[0] = self.terms[-1] = SENT
        d = Lb.GpMlpDesc()
        d.n_layers, d.n1, d.n2 = self.L, n1, self.n - n1
        d.flags = Lb.GPMLP_LOCKX if self.lockx else 0
        for k, w in enumerate(self.widths):
            d.width[k] = w
        for k in range(Lb.GPMLP_MAX_HIDDEN + 1):
            d.w[k] = off.get('W%d' % k, -1)
            d.b[k] = off.get('b%d' % k, -1)
        for k in range(Lb.GPMLP_MAX_HIDDEN):
            d.h[k] = woff.get('h%d' % (k + 1), -1)
            d.dh[k] = woff.get('dh%d' % (k + 1), -1)
        d.gp_ls = off['gp_ls']
        for name in ('qx_mu', 'qx_ls', 'qz_mu', 'qz_ls'):
            setattr(d, name, off[name])
            setattr(d, name + '2', off[name + '2'])
        for name in ('z', 'eps_z', 'eps_x', 'xs', 'mux', 'gxs', 'gmux', 'dz'):
            setattr(d, name, woff[name])
        d.lx_scale = self.segs[0][1]
        d.lx_scale2 = self.segs[1][1] if len(self.segs) > 1 else 0.0
        d.terms = self.terms.data_ptr() + 8
        d.terms2 = self.terms.data_ptr() + 8 + 16 * R
        self.desc = d
        return d

    def view(self, ws, name, width):
        o = self.woff[name]
        return ws[o:o + self.n * width].view(self.n, width).cpu().numpy()

    def owned_mask(self, names):
        m = torch.zeros(self.wsz, dtype=torch.bool)
        for name, width in names:
            m[self.woff[name]:self.woff[name] + self.n * width] = True
        return m

    def run(self, dev):
        """forward, backward, the weight-gradient GEMM -> (ws after forward, ws after backward, terms, gacc)."""
        from gpi import _lib as Lb
        lib = Lb.lib()
        d = self.desc
        ws = self.ws0.to(dev)
        self.terms[1:-1] = 0
        gacc = torch.zeros(self.P.numel(), dtype=torch.float64, device=dev)
        st = Lb.stream_handle()
        Lb.check(lib.gpi_gpmlp_forward(C.byref(d), Lb.ptr(self.P), Lb.ptr(ws), st), 'forward')
        ws_f = ws.clone()
        Lb.check(lib.gpi_gpmlp_backward(C.byref(d), Lb.ptr(self.P), Lb.ptr(ws), Lb.ptr(gacc), st), 'backward')
        items = []
        for k in range(1, self.L + 2):
            wo, wi = self.widths[k], self.widths[k - 1]
            a = self.woff['gmux'] if k == self.L + 1 else self.woff['dh%d' % k]
            b = self.woff['z'] if k == 1 else self.woff['h%d' % (k - 1)]
            items.append(Lb.GemmItem(a_off=a, b_off=b, c_off=self.off['W%d' % (k - 1)], bias_off=self.off['b%d' % (k - 1)],
                                     S=self.n, M=wo, N=wi, lda=wo, ldb=wi, flags=0))
        arr = (Lb.GemmItem * len(items))(*items)
        Lb.check(lib.gpi_outer_gemm(arr, len(items), Lb.ptr(ws), Lb.ptr(gacc), st), 'outer gemm')
        torch.cuda.synchronize()
        return ws_f.cpu(), ws.cpu(), self.terms.cpu().clone(), gacc.cpu()


SHAPES = [
    pytest.param([16, 24, 32], [(1, 1.0)], id='16-24-32_n1'),
    pytest.param([16, 24, 32], [(5, 1.0)], id='16-24-32_n5'),
    pytest.param([16, 21, 26, 32], [(4, 1.0)], id='16-21-26-32_n4'),
    pytest.param([64, 96, 128], [(32, 1.0), (4, 0.25)], id='64-96-128_n32+4'),
    pytest.param([64, 288, 512], [(3, 1.0)], id='64-288-512_n3'),
    pytest.param([16, 20, 24, 28, 32], [(2, 1.0)], id='16-20-24-28-32_n2'),
]


@pytest.mark.parametrize('lockx', [False, True], ids=['freeX', 'lockX'])
@pytest.mark.parametrize('widths,segs', SHAPES)
def test_forward_backward(device, widths, segs, lockx):
    from gpi import _lib as Lb
    c = Case(widths, segs, lockx, seed=7)
    c.layout(device)
    ref = c.ref
    ws_f, ws_b, terms, gacc = c.run(device)
    R, L, dx = Lb.GPI_REPLICAS, c.L, widths[-1]
    # ---- forward
    for k in range(1, L + 1):
        e = rel(c.view(ws_f, 'h%d' % k, widths[k]), ref['h'][k - 1].numpy())
        print('h%d' % k, e)
        assert e < 1e-5
        assert ((c.view(ws_f, 'h%d' % k, widths[k]) > 0) == (ref['h'][k - 1].numpy() > 0)).all()
    for name in ('mux', 'xs'):
        e = rel(c.view(ws_f, name, dx), ref[name].numpy())
        print(name, e)
        assert e < 1e-5
    owned = c.owned_mask([('h%d' % k, widths[k]) for k in range(1, L + 1)] + [('mux', dx), ('xs', dx)])
    assert torch.equal(ws_f[~owned], c.ws0[~owned]), 'the forward wrote outside h_k / mu_X / X~'
    assert terms[0] == SENT and terms[-1] == SENT
    t = terms[1:-1].view(2, 2, R).sum(2).numpy()         # [segment][logL_X, entropy]
    n1 = segs[0][0]
    if lockx:
        assert (t == 0).all()
    else:
        want = [[ref['logL_X'][:n1].sum(), ref['ent'][:n1].sum()], [ref['logL_X'][n1:].sum(), ref['ent'][n1:].sum()]]
        for s in range(len(segs)):
            for j in range(2):
                e = abs(t[s][j] - float(want[s][j])) / abs(float(want[s][j]))
                print('term', s, j, e)
                assert e < 1e-5
        if len(segs) == 1:
            assert (t[1] == 0).all()
    # ---- backward
    owned_b = c.owned_mask([('dh%d' % k, widths[k]) for k in range(1, L + 1)] + [('gmux', dx), ('dz', widths[0])])
    assert torch.equal(ws_b[~owned_b], ws_f[~owned_b]), 'the backward wrote outside delta_k / gmux / dz'
    got = {}
    g = lambda name, shape: gacc[c.off[name]:c.off[name] + int(np.prod(shape))].view(*shape).numpy()
    for k in range(L + 1):
        got['W%d' % k], got['b%d' % k] = g('W%d' % k, c.W[k].shape), g('b%d' % k, c.b[k].shape)
    seg_names = ['qz_mu', 'qz_ls'] + ([] if lockx else ['qx_mu', 'qx_ls'])
    for name in seg_names:
        w = widths[0] if name.startswith('qz') else dx
        got[name] = np.concatenate([g(name, (n1, w)), g(name + '2', (c.n - n1, w))])
    if not lockx:
        got['gp_ls'] = g('gp_ls', (dx,))
    assert sorted(got) == sorted(ref['grad'])
    for k, v in got.items():
        e = rel(v, ref['grad'][k].numpy())
        print('grad', k, e)
        assert e < 5e-5, k
    e = rel(c.view(ws_b, 'dz', widths[0]), ref['dz'].numpy())      # the optional W_1^T delta_1 output
    print('dz', e)
    assert e < 5e-5
    # everything of gacc that is no gradient of this op stays zero
    used = torch.zeros(gacc.numel(), dtype=torch.bool)
    for name, tt in [('W%d' % k, c.W[k]) for k in range(L + 1)] + [('b%d' % k, c.b[k]) for k in range(L + 1)]:
        used[c.off[name]:c.off[name] + tt.numel()] = True
    for name in ('qz_mu', 'qz_ls', 'qx_mu', 'qx_ls'):
        w = widths[0] if name.startswith('qz') else dx
        used[c.off[name]:c.off[name] + n1 * w] = True
        used[c.off[name + '2']:c.off[name + '2'] + (c.n - n1) * w] = True
    used[c.off['gp_ls']:c.off['gp_ls'] + dx] = True
    assert (gacc[~used] == 0).all()
    # ---- a second run gives the same bits
    ws_f2, ws_b2, terms2, gacc2 = c.run(device)
    assert torch.equal(ws_f, ws_f2) and torch.equal(ws_b, ws_b2) and torch.equal(gacc, gacc2)
    assert torch.equal(terms, terms2)


def test_more_than_three_hidden_layers_is_refused(device):
    from gpi import _lib as Lb
    lib = Lb.lib()
    c = Case([16, 24, 32], [(2, 1.0)], False, seed=1)
    d = c.layout(device)
    ws = c.ws0.to(device)
    gacc = torch.zeros(c.P.numel(), dtype=torch.float64, device=device)
    d.n_layers = 4
    assert lib.gpi_gpmlp_forward(C.byref(d), Lb.ptr(c.P), Lb.ptr(ws), None) == -3       # GPI_ERR_UNSUPPORTED
    assert lib.gpi_gpmlp_backward(C.byref(d), Lb.ptr(c.P), Lb.ptr(ws), Lb.ptr(gacc), None) == -3
    s = Lb.GpMlpSampleDesc(rows=1, rep=1, n_layers=4)
    assert lib.gpi_gpmlp_sample(C.byref(s), None) == -3
    d.n_layers = 0
    assert lib.gpi_gpmlp_forward(C.byref(d), Lb.ptr(c.P), Lb.ptr(ws), None) == -1       # L = 0 is the head's
    torch.cuda.synchronize()
    assert torch.equal(ws.cpu(), c.ws0) and (gacc == 0).all()
    # absent (-1) workspace buffers of a used layer, and sampling noise without its draw, are argument errors
    d.n_layers = 1
    for name in ('z', 'mux', 'eps_x'):
        keep = getattr(d, name)
        setattr(d, name, -1)
        assert lib.gpi_gpmlp_forward(C.byref(d), Lb.ptr(c.P), Lb.ptr(ws), None) == -1, name
        setattr(d, name, keep)
    keep, d.h[0] = d.h[0], -1
    assert lib.gpi_gpmlp_forward(C.byref(d), Lb.ptr(c.P), Lb.ptr(ws), None) == -1
    d.h[0] = keep
    keep, d.dh[0] = d.dh[0], -1
    assert lib.gpi_gpmlp_backward(C.byref(d), Lb.ptr(c.P), Lb.ptr(ws), Lb.ptr(gacc), None) == -1
    d.dh[0] = keep
    p = Lb.ptr(c.P)
    s = Lb.GpMlpSampleDesc(rows=5, rep=2, n_layers=1, qz_mu=p.value, x=p.value)
    s.width[0], s.width[1], s.width[2] = 16, 24, 32
    for k in range(2):
        s.w[k] = s.b[k] = p.value
    assert lib.gpi_gpmlp_sample(C.byref(s), None) == -1                                # rows no multiple of rep
    s.rows, s.eps_z = 4, p.value
    assert lib.gpi_gpmlp_sample(C.byref(s), None) == -1                                # eps_z without q logsigma
    torch.cuda.synchronize()
    assert torch.equal(ws.cpu(), c.ws0) and (gacc == 0).all()
    # the Python layers raise with a clear message
    from gpi.engine import check_gp_hidden
    with pytest.raises(Lb.NativeError, match='at most 3'):
        check_gp_hidden(4)


def _net(widths, seed, dev):
    from lamp.neuralnets import FeedforwardNeuralNetwork
    torch.manual_seed(seed)
    return FeedforwardNeuralNetwork(widths[0], widths[-1], widths[1:-1], None, dtype=torch.float32, device=dev)


@pytest.mark.parametrize('widths,N,rep', [([16, 24, 32], 3, 5), ([16, 21, 26, 32], 2, 9), ([64, 288, 512], 2, 2)])
def test_sampling_on_injected_noise(device, widths, N, rep):
    """x = mlp(q mean[r / rep] + exp(q logsigma[r / rep]) eps_z) + exp(logsigmas_X) eps_x vs fp64 torch at 1e-5; the
    mean-only form (no q logsigma, no logsigmas_X)."""
    from gpi.predictive import gp_mlp_sample
    net = _net(widths, 3, device)
    g = torch.Generator().manual_seed(11)
    dz, dx, rows = widths[0], widths[-1], N * rep
    mu, ls = 0.5 * torch.randn(N, dz, generator=g), -1 + 0.3 * torch.randn(N, dz, generator=g)
    ez, ex = torch.randn(rows, dz, generator=g), torch.randn(rows, dx, generator=g)
    gls = -0.5 + 0.2 * torch.randn(dx, generator=g)
    Ws = [fc.weight.detach().double().cpu() for fc in net.linears]
    bs = [fc.bias.detach().double().cpu() for fc in net.linears]
    z = (mu.double() + torch.exp(ls.double()) * ez.double().view(N, rep, dz).transpose(0, 1)).transpose(0, 1).reshape(rows, dz)
    pre = []
    want, _ = mlp64(Ws, bs, z, pre)
    x = torch.full((rows + 1, dx), SENT, device=device)
    cu = lambda t: t.to(device).contiguous()
    gp_mlp_sample(net.linears, cu(mu), cu(ls), cu(gls), x[:rows], rep=rep, eps_z=cu(ez), eps_x=cu(ex))
    torch.cuda.synchronize()
    # (rows whose hidden pre-activations sit within fp32 rounding of zero would need the kernel's decision: none
    # at this margin)
    assert min(float(a.abs().min()) for a in pre) > 1e-5
    assert rel(x[:rows].cpu().numpy(), (want + torch.exp(gls.double()) * ex.double()).numpy()) < 1e-5
    assert (x[rows] == SENT).all()
    xm = torch.empty(N, dx, device=device)
    gp_mlp_sample(net.linears, cu(mu), None, None, xm)
    torch.cuda.synchronize()
    assert rel(xm.cpu().numpy(), mlp64(Ws, bs, mu.double())[0].numpy()) < 1e-5


def test_sampling_philox_row_repeat_layout(device):
    """Philox draws: with q logsigma = -inf the draw is the q mean of row r / rep whatever the normals are (the
    layout); with logsigmas_X the residual x - mlp(mean) is exp(logsigmas_X) times unit normals; a seed fixes the
    draw, another seed changes it."""
    from gpi.predictive import gp_mlp_sample
    widths, N, rep = [16, 24, 32], 16, 1024             # 16 384 rows, the VO update's predictive
    net = _net(widths, 5, device)
    g = torch.Generator().manual_seed(13)
    mu = (0.5 * torch.randn(N, 16, generator=g)).to(device)
    ninf = torch.full((N, 16), -float('inf'), device=device)
    x = torch.empty(N * rep, 32, device=device)
    gp_mlp_sample(net.linears, mu, ninf, None, x, rep=rep, seed=99)
    with torch.no_grad():
        want = net(mu)
    torch.cuda.synchronize()
    got = x.view(N, rep, 32)
    assert torch.equal(got, got[:, :1].expand(-1, rep, -1)), 'rows of one q row differ'
    assert rel(got[:, 0].cpu().numpy(), want.cpu().numpy()) < 1e-5
    gls = torch.full((32,), -1.0, device=device)
    xa, xb, xc = (torch.empty(N * rep, 32, device=device) for _ in range(3))
    gp_mlp_sample(net.linears, mu, ninf, gls, xa, rep=rep, seed=99)
    gp_mlp_sample(net.linears, mu, ninf, gls, xb, rep=rep, seed=99)
    gp_mlp_sample(net.linears, mu, ninf, gls, xc, rep=rep, seed=100)
    torch.cuda.synchronize()
    assert torch.equal(xa, xb) and not torch.equal(xa, xc)
    e = ((xa - x) / math.exp(-1.0)).double()
    # 524 288 unit normals: mean within 5 sigma / sqrt(n), variance within 5 sqrt(2 / n)
    n = e.numel()
    assert abs(float(e.mean())) < 5 / math.sqrt(n) and abs(float(e.var()) - 1) < 5 * math.sqrt(2 / n)
    # q_z noise: z varies within a q row once logsigma is finite
    xz = torch.empty(N * rep, 32, device=device)
    gp_mlp_sample(net.linears, mu, torch.full((N, 16), -1.0, device=device), None, xz, rep=rep, seed=99)
    torch.cuda.synchronize()
    assert not torch.equal(xz.view(N, rep, 32)[:, 0], xz.view(N, rep, 32)[:, 1])
