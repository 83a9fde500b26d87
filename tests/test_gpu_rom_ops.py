"""Operator-level sweep of the coarse-grained model: gpi_rom in every kernel form and mode against the fp64
reference (tests/rom_ref.py) over the case table of tests/rom_cases.py, launched through the raw descriptor.

Per case, against fp64 (the project's max|d| / max|ref|): uc, mu_y 1e-5, |L - L_ref| <= 1e-5 |L_ref| (the sum and
every sample's replica slot), gx 1e-4, d/dlogsigma_y 1e-5 (the gacc_logsig sum, the gls_part rows and their sum).
Exact properties:
  * every output buffer starts as a NaN bit pattern no kernel produces, with two more rows behind row N and, for the
    strided ones, padding columns: every entry the mode owns is written, everything else keeps the pattern (the fp64
    accumulators: a sentinel tail); flag stays 0 in every launch but the flagged one;
  * loglik: the gls_part launch gives the bits of the gacc_logsig launch in uc, mu_y, gx and loss_acc; sample s adds
    to loss_acc[s % GPI_REPLICAS] and to no other slot;
  * N = 3 shapes: every row has the bits of the N = 1 launch of that row (uc, mu_y, gx, gls_part);
  * x_draw: the launch that draws x in the kernel (rows at a padded stride, NaN in the padding) equals the stored-x
    launch on the exactly computed sample, bit for bit;
  * gx_acc: gx_accumulate into a pre-filled buffer at a padded stride stays within the FMA bound 2^-22 (|pre| + |g|)
    of pre + g and leaves the padding alone;
  * loss_scale = 0.25 leaves the bits of loss_acc;
  * flag: one kappa <= 1e-12 in one row sets flag to 1 and leaves the bits of the other rows;
  * coarse: uc within 2e-6 of the full forward's uc, and every row of it within 1e-5 of fp64.
Dispatch arms the environment selects (read once per process: one child process per arm, each writing its raw
outputs to an .npz the parent compares): GPI_ROM_FAST_NT=256 and =1024 over the nc = 8 part of the table,
GPI_ROM_SLOW=1 over the nc = 4 and nc = 8 parts; the same fp64 bars, and the 256 / 512 / 1024 arms within 2e-5 (mu)
and 2e-4 (gx) of each other.

Each test prints its measured maxima per quantity (profiles/rom_ops_parity.txt)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, PKG
import rom_cases as T
import rom_ref as R
from rom_cases import rom_desc

pytestmark = pytest.mark.gpu
TESTS = os.path.dirname(os.path.abspath(__file__))
POISON_BITS = 0x7FC5A5A5          # a quiet NaN no kernel produces
PAD_ROWS = 2
SENTINEL = -7.0                   # tail of the fp64 accumulators
BAR = dict(T.BAR, gls_part_sum=1e-5)


def cuda(a, dtype=torch.float32):
    return torch.tensor(np.asarray(a), dtype=dtype, device='cuda')


def poison(*shape):
    return torch.full(shape, POISON_BITS, dtype=torch.int32, device='cuda').view(torch.float32)


def is_poison(t):
    return t.contiguous().view(torch.int32) == POISON_BITS


def bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def strided(a, stride, fill=None):
    """Rows of `a` [N, w] at `stride` floats, the padding poisoned (or `fill`)."""
    N, w = a.shape
    out = poison(N, stride) if fill is None else fill.clone()
    out[:, :w] = a
    return out


def launch(c, inp, N, form='part', draw=False, pre=None, loss_scale=None, poke=None, coarse=None):
    """One gpi_rom launch of case c's mode on the inputs `inp` (N rows) -> dict of the written outputs (tensors).
    form: loglik's gradient sink ('part' rows or the 'gacc' sum); draw: x drawn in the kernel; pre: [N, stride]
    values gx accumulates into; poke: (row, entry) of a kappa set to 1e-13; coarse: override of the case's
    coarse-only form."""
    from gpi import _lib as L
    nc, r, D = c.nc, c.r, c.dims
    nT, nn, dy = D['nT'], D['nn'], D['dy']
    mode = c.mode
    coarse = (mode == 'coarse') if coarse is None else coarse
    kw = dict(input_kappa=int(c.input_kappa))
    x = cuda(inp['x'])
    if poke is not None:
        x[poke[0], poke[1]] = 1e-13
    if draw:
        xs = nT + 24
        kw.update(x_draw=1, x_mu=strided(cuda(inp['x_mu']), xs), x_ls=strided(cuda(inp['x_ls']), xs),
                  x_eps=strided(cuda(inp['x_eps']), xs), x_stride=xs)
        kw['x'] = kw['x_mu']
    else:
        kw.update(x=x, x_stride=nT)
    flag = torch.zeros(1 + 4, dtype=torch.int32, device='cuda')
    kw.update(F=cuda(inp['F']), flag=flag)
    out, rows = {}, N + PAD_ROWS
    if mode in ('forward', 'coarse', 'loglik'):
        out['uc'] = kw['uc'] = poison(rows, nn)
        if not coarse:
            out['mu'] = kw['mu_y'] = poison(rows, dy)
    gs = nT
    if mode not in ('forward', 'coarse'):
        if pre is not None:
            gs = pre.shape[1]
            out['gx'] = poison(rows, gs)
            out['gx'][:N] = pre
            kw['gx_accumulate'] = 1
        else:
            out['gx'] = poison(rows, gs)
        kw.update(gx=out['gx'], gx_stride=gs)
    if mode == 'loglik':
        acc = torch.full((T.REPLICAS + 8,), SENTINEL, dtype=torch.float64, device='cuda')
        acc[:T.REPLICAS] = 0
        if form == 'part':
            out['gls'] = kw['gls_part'] = poison(rows, dy)
        else:
            out['gls'] = torch.full((dy + 8,), SENTINEL, dtype=torch.float64, device='cuda')
            out['gls'][:dy] = 0
            kw['gacc_logsig'] = out['gls']
        out['acc'] = acc
        kw.update(Y=cuda(inp['Y']), logsig_y=cuda(inp['ls']), loss_acc=acc,
                  loss_scale=c.loss_scale if loss_scale is None else loss_scale)
        lmode = L.ROM_LOGLIK
    elif mode in ('forward', 'coarse'):
        lmode = L.ROM_FORWARD
    else:
        lmode = L.ROM_BACKWARD
        if mode in ('bwd_dmu', 'bwd_both'):
            kw['dmu'] = cuda(inp['dmu'])
        if mode in ('bwd_duc', 'bwd_both'):
            kw['duc'] = cuda(inp['duc'])
    rom_desc(nc, r, N, lmode, **kw)
    # what the launch must not touch, and what it must have written
    assert flag[0].item() == int(poke is not None), (c.id, 'flag', flag.tolist())
    assert (flag[1:] == 0).all()
    res = {'flag': int(flag[0].item())}
    for k, t in out.items():
        if t.dtype == torch.float64:
            n = T.REPLICAS if k == 'acc' else dy
            assert (t[n:] == SENTINEL).all(), (c.id, k, 'tail written')
            res[k] = t[:n].clone()
            continue
        assert is_poison(t[N:]).all(), (c.id, k, 'rows past N written')
        w = nT if k == 'gx' else t.shape[1]
        if k == 'gx' and gs > nT:
            keep = pre[:, nT:] if pre is not None else t[:N, nT:]
            assert same_bits(t[:N, nT:], keep), (c.id, 'gx padding written')
        assert not torch.isnan(t[:N, :w]).any(), (c.id, k, 'entries the mode owns are not written')
        res[k] = t[:N, :w].clone()
    return res


def rows_of(inp, i):
    """The inputs of row i alone."""
    d = dict(inp)
    for k in ('x', 'F', 'Y', 'dmu', 'duc', 'x_mu', 'x_ls', 'x_eps'):
        if k in d:
            d[k] = d[k][i:i + 1]
    return d


def run_case(c):
    """Every launch of one case and its exact properties -> the outputs to compare with fp64 (numpy arrays)."""
    inp, N = c.inputs(), c.N
    a = launch(c, inp, N)
    got = {k: a[k] for k in ('uc', 'mu', 'gx') if k in a}
    if c.mode == 'loglik':
        b = launch(c, inp, N, form='gacc')
        for k in ('uc', 'mu', 'gx', 'acc'):
            assert same_bits(a[k], b[k]), (c.id, k, 'gls_part form vs gacc_logsig form')
        got.update(gls=b['gls'], gls_rows=a['gls'], gls_part_sum=a['gls'].double().sum(0))
        acc = a['acc']
        assert N <= T.REPLICAS and (acc[N:] == 0).all() and (acc[:N] != 0).all(), (c.id, 'replica slots', acc.tolist())
        got.update(L=acc.sum().item(), L_rows=acc[:N])
        if c.opt == 'loss_scale':
            one = launch(c, inp, N, loss_scale=1.0)
            assert same_bits(one['acc'], acc), (c.id, 'loss_scale changed the value')
            assert not same_bits(one['gx'], a['gx'])
    if N == 3 and c.opt is None:
        for i in range(N):
            ai = launch(c, rows_of(inp, i), 1)
            for k in ('uc', 'mu', 'gx', 'gls'):
                if k in a:
                    assert same_bits(ai[k][0], a[k][i]), (c.id, k, 'row %d depends on its batch mates' % i)
    if c.opt == 'x_draw':
        b = launch(c, inp, N, draw=True)
        for k in a:
            if k != 'flag':
                assert same_bits(a[k], b[k]), (c.id, k, 'x drawn in the kernel vs the stored sample')
    if c.opt == 'gx_acc':
        nT = c.dims['nT']
        pre = cuda(np.random.default_rng(c.index).normal(size=(N, nT + 8)))
        b = launch(c, inp, N, pre=pre)
        # the kernel adds its last product into the buffer as one FMA (contraction), the stored form rounds the
        # product first: at most half an ulp of the term plus one rounding of the sum apart
        want = pre[:, :nT].double() + a['gx'].double()
        bound = 2.0 ** -22 * (pre[:, :nT].abs() + a['gx'].abs()).double()
        assert ((b['gx'].double() - want).abs() <= bound).all(), (c.id, 'gx_accumulate')
        assert not same_bits(b['gx'], pre[:, :nT])
        for k in a:
            if k not in ('gx', 'flag'):
                assert same_bits(a[k], b[k]), (c.id, k, 'gx_accumulate changed another output')
    if c.opt == 'flag':
        row = inp['poke'][0]
        b = launch(c, inp, N, poke=inp['poke'])
        others = [i for i in range(N) if i != row]
        assert others
        for k in ('uc', 'mu'):
            if k in a:
                assert same_bits(a[k][others], b[k][others]), (c.id, k, 'the flagged row changed its batch mates')
    if c.mode == 'coarse':
        full = launch(c, inp, N, coarse=False)
        e = R.rel_err(a['uc'].cpu(), full['uc'].cpu().numpy().astype(np.float64))
        assert e < T.CROSS_BAR, (c.id, 'coarse-only uc vs the full forward', e)
    return {k: (v if isinstance(v, float) else v.cpu().numpy()) for k, v in got.items()}


def errors(c, got):
    ref = c.reference()
    errs = T.compare(got, ref)
    if 'gls_part_sum' in got:
        errs['gls_part_sum'] = R.rel_err(got['gls_part_sum'], ref['gls'])
    if c.mode == 'coarse':      # every row on its own
        errs['uc'] = max([errs['uc']] + [R.rel_err(got['uc'][i], ref['uc'][i]) for i in range(c.N)])
    return errs


def check(cs, run, tag):
    """run(case) -> outputs, compared with fp64 for every case of cs; prints and returns the worst per quantity."""
    W = {}
    assert cs
    for c in cs:
        errs = errors(c, run(c))
        bad = {k: e for k, e in errs.items() if not e < BAR[k] and not (k in ('L', 'L_rows') and e <= BAR[k])}
        assert not bad, (tag, c.id, bad)
        for k, e in errs.items():
            if k not in W or e > W[k][0]:
                W[k] = (e, c.id)
    print('ROMOPS %s (%d cases) ' % (tag, len(cs)) + ' '.join('%s=%.2e(%s)' % ((k,) + W[k]) for k in sorted(W)))
    return W


ITEMS = [(f, m) for f in T.FULL_FAMILIES for m in T.MODES] + [(f, 'coarse') for f in T.COARSE_NC]


@pytest.mark.parametrize('family,mode', ITEMS, ids=['%s-%s' % i for i in ITEMS])
def test_rom_ops_vs_fp64(device, family, mode):
    """Every case of one kernel family in one mode, options included (module docstring)."""
    W = check(T.select(family, mode), run_case, '%s %s' % (family, mode))
    want = {'forward': {'uc', 'mu'}, 'coarse': {'uc'},
            'loglik': {'uc', 'mu', 'L', 'L_rows', 'gx', 'gls', 'gls_rows', 'gls_part_sum'}}.get(mode, {'gx'})
    assert set(W) == want


def test_items_cover_the_table():
    assert sorted(c.index for f, m in ITEMS for c in T.select(f, m)) == list(range(len(T.cases())))


# ---------------------------------------------------------------------- refusals
def test_rom_refusals_and_empty_batch(device):
    """Return codes only: nc = 1 / 17, refine = 0, LOGLIK without Y / logsig_y / both gradient sinks / gx, BACKWARD
    with neither dmu nor duc / without gx; n = 0 returns OK and writes nothing."""
    from gpi import _lib as L
    OK, ERR_ARG = 0, -1
    buf = poison(4096)

    def rc(mode, nc=4, refine=2, n=1, **kw):
        a = dict(x=buf, F=buf, Y=buf, logsig_y=buf, gx=buf, gls_part=buf, gacc_logsig=buf, dmu=buf, duc=buf,
                 mu_y=buf, uc=buf, loss_acc=buf, flag=buf, x_stride=2 * nc * nc, gx_stride=2 * nc * nc, check=False)
        a.update(kw)
        return rom_desc(nc, refine, n, mode, **a)

    for mode in (L.ROM_FORWARD, L.ROM_LOGLIK, L.ROM_BACKWARD):
        assert rc(mode, nc=1) == ERR_ARG and rc(mode, nc=17) == ERR_ARG
        assert rc(mode, refine=0) == ERR_ARG
        assert rc(mode, n=0) == OK
        for nc in (2, 7, 8, 16):
            assert rc(mode, nc=nc, n=0) == OK
    for k in ('Y', 'logsig_y', 'gx'):
        assert rc(L.ROM_LOGLIK, **{k: 0}) == ERR_ARG, k
    assert rc(L.ROM_LOGLIK, gls_part=0, gacc_logsig=0) == ERR_ARG
    assert rc(L.ROM_BACKWARD, dmu=0, duc=0) == ERR_ARG
    assert rc(L.ROM_BACKWARD, gx=0) == ERR_ARG
    assert rc(L.ROM_FORWARD, mu_y=0, n=0) == OK
    assert is_poison(buf).all()


# ---------------------------------------------------------------------- dispatch arms of the environment
ARMS = {'nt256': ({'GPI_ROM_FAST_NT': '256'}, (8,)), 'nt1024': ({'GPI_ROM_FAST_NT': '1024'}, (8,)),
        'slow': ({'GPI_ROM_SLOW': '1'}, (4, 8))}
ARM_VARS = ('GPI_ROM_FAST_NT', 'GPI_ROM_SLOW')
_ARM = {}

CHILD = '''
import sys
for p in (%r, %r, %r):
    sys.path.insert(0, p)
import test_gpu_rom_ops as G
G.child(sys.argv[1], sys.argv[2])
'''


def arm_cases(name):
    return T.select(nc=ARMS[name][1])


def child(name, path):
    """In the child process of one arm: every launch and exact property of its cases; raw outputs to `path`."""
    env = ARMS[name][0]
    assert all(os.environ.get(k) == env.get(k) for k in ARM_VARS), os.environ
    out = {}
    for c in arm_cases(name):
        for k, v in run_case(c).items():
            out['%d:%s' % (c.index, k)] = np.asarray(v)
    np.savez(path, **out)
    print('ROMOPS child %s: %d cases' % (name, len(arm_cases(name))))


def arm(name, tmp_path_factory):
    """case index -> outputs of one arm (its child process runs once per session)."""
    if name not in _ARM:
        env = {k: v for k, v in os.environ.items() if k not in ARM_VARS}
        env.update(ARMS[name][0])
        path = str(tmp_path_factory.mktemp('rom_ops') / (name + '.npz'))
        r = subprocess.run([sys.executable, '-c', CHILD % (TESTS, ROOT, PKG), name, path], env=env,
                           capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, (name, r.stdout[-2000:], r.stderr[-3000:])
        assert 'ROMOPS child' in r.stdout
        z = np.load(path)
        res = {}
        for key in z.files:
            i, k = key.split(':')
            v = z[key]
            res.setdefault(int(i), {})[k] = float(v) if v.ndim == 0 else v
        _ARM[name] = res
    return _ARM[name]


def default_arm():
    if 'nt512' not in _ARM:
        _ARM['nt512'] = {c.index: run_case(c) for c in T.select(nc=(4, 8))}
    return _ARM['nt512']


@pytest.mark.parametrize('name', list(ARMS))
def test_rom_ops_dispatch_arm(device, tmp_path_factory, name):
    """One arm's child process over its part of the table: the fp64 bars on what it wrote, and a kernel other than
    the default one (some bit of some gx differs from the default arm's)."""
    res = arm(name, tmp_path_factory)
    cs = arm_cases(name)
    assert sorted(res) == [c.index for c in cs]
    for fam in sorted({c.family for c in cs}):
        check([c for c in cs if c.family == fam], lambda c: res[c.index], '%s %s' % (name, fam))
    ref = default_arm()
    full = [c for c in cs if 'gx' in res[c.index]]
    assert any(not np.array_equal(res[c.index]['gx'], ref[c.index]['gx']) for c in full), name


def test_rom_ops_workgroup_widths_agree(device, tmp_path_factory):
    """rom_kernel_fast<8, 256 | 512 | 1024> on the nc = 8 part of the table: within 2e-5 (mu) and 2e-4 (gx) of each
    other, the bars of the nc = 16 cross-kernel test."""
    arms = {'nt256': arm('nt256', tmp_path_factory), 'nt512': default_arm(), 'nt1024': arm('nt1024', tmp_path_factory)}
    worst = {}
    for c in T.select(nc=(8,)):
        for a, b in (('nt256', 'nt512'), ('nt1024', 'nt512'), ('nt256', 'nt1024')):
            for k, bar in (('mu', 2e-5), ('gx', 2e-4)):
                if k in arms[a][c.index]:
                    e = R.rel_err(arms[a][c.index][k], arms[b][c.index][k])
                    assert e < bar, (c.id, a, b, k, e)
                    key = '%s/%s %s' % (a, b, k)
                    worst[key] = max(worst.get(key, (0.0, None)), (e, c.id))
    print('ROMOPS widths ' + ' '.join('%s=%.2e(%s)' % ((k,) + worst[k]) for k in sorted(worst)))
