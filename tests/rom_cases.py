"""Case table of the coarse-grained model's operator sweep (tests/test_rom_cases_plan.py on the CPU,
tests/test_gpu_rom_ops.py on the GPU).  Imports without a GPU.

A case is (family, nc, r, N, mode, option).  Families are the kernels gpi_rom dispatches to:
    fast4 / fast8 / fast16   rom_kernel_fast<4,256>, <8,512> (<8,256>, <8,1024> by GPI_ROM_FAST_NT), <16,512>
    generic                  rom_kernel: every other nc <= 16 (and nc = 4, 8, 16 under GPI_ROM_SLOW=1)
    lane4 / lane8            rom_lane_kernel<4 | 8>: FORWARD with uc and without mu_y, one lane per sample
    coarse16                 rom16_coarse_kernel: the same at nc = 16, one wave per sample
Modes: forward (mu_y + uc), loglik (run in the gacc_logsig and in the gls_part form), bwd_dmu, bwd_duc, bwd_both,
coarse (uc only; family generic: rom_kernel's early return).
Shapes, the smallest at which each form can still go wrong:
    native forms      nc in {4, 8, 16} x r in {1, 2, 3, 5} x N in {1, 3}, and (4, 7), (8, 7) at N = 3
                      (r = 1, 2: the first coarse column has 0 / 1 fine columns per square and squares have fewer
                      nodes than threads; odd r: P1 weights at thirds, fifths, sevenths, e / ncol by the reciprocal
                      multiply at ncol 2..7)
    generic           nc in {2, 3, 6, 7, 11, 15} x r in {1, 3} at N = 2, and (2, 2), (15, 2)
    coarse            lane4 / lane8 at N in {1, 63, 64, 65, 130}, coarse16 at N in {1, 2, 3}, generic nc = 7 at N = 2
Options, each on one shape per family ((nc, 3, 3) for the native forms, (7, 3, 2) for the generic kernel, N = 3 for
the coarse-only families):
    kappa        input_kappa = 1: forward, bwd_both, coarse
    kappa_tiny   the same with every kappa scaled by 2^-25 (kappa ~ 3e-8, far above the 1e-12 of the flag): the
                 solution is invariant under the scaling, and only here would a stray + 1e-8 show
    x_draw       the q_X sample drawn in the kernel, rows at x_stride = 2 nc^2 + 24, log-sigmas in {0, -inf} (expf
                 exact in every implementation): loglik, coarse
    gx_acc       gx_stride = 2 nc^2 + 8, gx_accumulate = 1 into a pre-filled buffer: loglik, bwd_dmu
    loss_scale   0.25: loglik
    flag         one kappa entry of one row <= 1e-12 under input_kappa: forward, coarse
    contrast     x ~ N(0, 1.5^2), r = 2, N = 5: every mode
Values: x ~ N(0.3, 0.7^2), Dirichlet values U(-0.5, 0.5) on the left and right coarse columns, logsigma_y =
log 0.3 + 0.1 eps, Y = mu_fp64 + 0.3 eps, dmu, duc ~ N(0, 1), seeded per (nc, r, N, option): the modes of a shape
share their inputs (DRAW: the two contrast draws that are not the first of their seed).
"""
import functools
import zlib

import numpy as np

import rom_ref as R

REPLICAS = 16                    # GPI_REPLICAS of the library build (gpi/_lib.py checks it at load)
# the operator bars (max|d| / max|ref|; L, L_rows: |d| / |ref| per value)
BAR = {'uc': 1e-5, 'mu': 1e-5, 'L': 1e-5, 'L_rows': 1e-5, 'gls': 1e-5, 'gls_rows': 1e-5, 'gx': 1e-4}

FAMILIES = ('fast4', 'fast8', 'fast16', 'generic', 'lane4', 'lane8', 'coarse16')
FULL_FAMILIES = FAMILIES[:4]
MODES = ('forward', 'loglik', 'bwd_dmu', 'bwd_duc', 'bwd_both')
OPTIONS = ('kappa', 'kappa_tiny', 'x_draw', 'gx_acc', 'loss_scale', 'flag', 'contrast')
KAPPA_OPTS = ('kappa', 'kappa_tiny', 'flag')
OPTION_MODES = {'kappa': ('forward', 'bwd_both'), 'kappa_tiny': ('forward', 'bwd_both'), 'x_draw': ('loglik',),
                'gx_acc': ('loglik', 'bwd_dmu'), 'loss_scale': ('loglik',), 'flag': ('forward',), 'contrast': MODES}
COARSE_OPTIONS = ('kappa', 'x_draw', 'flag', 'contrast')
TAGS = ('odd_r', 'r1', 'ncol01', 'umulhi', 'nc2', 'duc', 'kappa', 'ragged_wave', 'poison') + R.WRONG
TINY = 2.0 ** -25
CROSS_BAR = 2e-6                 # coarse-only uc vs the full forward's uc (two fp32 kernels)
# Draws that are not the first of their seed sequence.  A draw must leave the bars attainable for an fp32 kernel
# (tests/test_rom_cases_plan.py): the fp32 dense solve of the same systems within a quarter of the fp64 bars and, at
# nc = 4 and 8 where the coarse-only form is another algorithm than the full forward, within half of CROSS_BAR in
# uc (two fp32 solves, half the bar each).  The draws at the standard statistics are taken as they come (<= 1.0e-6,
# and <= 6.6e-7 at nc = 4, 8).  The contrast draws are walked to the first one that meets both conditions with room
# for another machine's BLAS: (16, 2, 5) draws 0 and 1 have the dense fp32 solve 1.6e-6 .. 2.0e-6 from fp64 in uc
# and mu (a quarter of the bar is 2.5e-6), draw 2 1.0e-6 / 1.2e-6; (8, 2, 5) draws 0 .. 3 have it at
# 6.0e-7 .. 3.5e-6, draw 4 at 3.9e-7.  (On draw 1 of (8, 2, 5), 6.0e-7, rom_lane_kernel<8> is 2.4e-6 and
# rom_kernel_fast<8, 512> 8.2e-7 from fp64 and 3.2e-6 from each other; on the other nine of ten draws measured the
# two are 4.7e-7 .. 1.0e-6 apart: profiles/rom_ops_parity.txt.)  Fixed here, not walked at run time, so that every
# machine tests the same inputs.
DRAW = {(16, 2, 5, 'contrast'): 2, (8, 2, 5, 'contrast'): 4}


def family_of(nc, coarse=False):
    if coarse:
        return {4: 'lane4', 8: 'lane8', 16: 'coarse16'}.get(nc, 'generic')
    return {4: 'fast4', 8: 'fast8', 16: 'fast16'}.get(nc, 'generic')


def dims(nc, r):
    n = nc * r
    return dict(nn=(nc + 1) ** 2, nT=2 * nc * nc, dy=(n + 1) * (n - 1))


@functools.lru_cache(maxsize=None)
def inputs(nc, r, N, opt):
    """The fp32 inputs of every mode of one (shape, option), as float32 arrays:
    x (what the kernel solves with: x, kappa with the kappa options, the exactly computed draw with x_draw), F, ls,
    Y, dmu, duc; x_draw: x_mu, x_ls, x_eps [N, nT] besides; flag: poke = (row, entry).
    The draw is number DRAW[(nc, r, N, opt)] of its seed sequence, 0 unless listed there."""
    return _draw(nc, r, N, opt, DRAW.get((nc, r, N, opt), 0))


def _draw(nc, r, N, opt, attempt):
    D = dims(nc, r)
    rng = np.random.default_rng(zlib.crc32(('%d-%d-%d-%s-%s' % (nc, r, N, opt, attempt)).encode()))
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    m, s = (0.0, 1.5) if opt == 'contrast' else (0.3, 0.7)
    x = f32(rng.normal(m, s, (N, D['nT'])))
    F = np.zeros((N, D['nn']), dtype=np.float32)
    bn = [e for e in range(D['nn']) if e % (nc + 1) in (0, nc)]
    F[:, bn] = rng.uniform(-0.5, 0.5, (N, len(bn)))
    ls = f32(np.log(0.3) + 0.1 * rng.normal(size=D['dy']))
    eps_y = rng.normal(size=(N, D['dy']))
    d = dict(F=F, ls=ls, dmu=f32(rng.normal(size=(N, D['dy']))), duc=f32(rng.normal(size=(N, D['nn']))))
    if opt in KAPPA_OPTS:
        x = f32(np.exp(x.astype(np.float64)) + 1e-8)
        if opt == 'kappa_tiny':
            x = x * np.float32(TINY)            # a power of two: exact
        if opt == 'flag':
            d['poke'] = (N // 2, 7 % D['nT'])
    if opt == 'x_draw':
        d['x_mu'] = x
        d['x_ls'] = f32(np.where(rng.random((N, D['nT'])) < 0.5, 0.0, -np.inf))
        d['x_eps'] = f32(0.05 * rng.normal(size=(N, D['nT'])))
        # fmaf(expf(ls), eps, mu) in fp32: exact product and sum in fp64 (24-bit operands), rounded once
        x = f32(np.exp(d['x_ls'].astype(np.float64)) * d['x_eps'].astype(np.float64) + x.astype(np.float64))
        assert not np.array_equal(x, d['x_mu'])
    d['x'] = x
    ref = R.forward(nc, r, x, F, input_kappa=opt in KAPPA_OPTS)
    d['uc64'], d['mu64'] = ref['uc'], ref['mu']
    d['Y'] = f32(ref['mu'] + 0.3 * eps_y)
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


class Case:
    def __init__(self, index, nc, r, N, mode, opt=None):
        self.index, self.nc, self.r, self.N, self.mode, self.opt = index, nc, r, N, mode, opt
        self.family = family_of(nc, mode == 'coarse')
        self.id = '%s-nc%d_r%d_N%d-%s%s' % (self.family, nc, r, N, mode, '-' + opt if opt else '')
        self.input_kappa = opt in KAPPA_OPTS
        self.loss_scale = 0.25 if opt == 'loss_scale' else 1.0
        self.dims = dims(nc, r)
        uses_mu = mode in ('forward', 'loglik', 'bwd_dmu', 'bwd_both')
        t = {'no_lift', 'poison'}
        if r >= 3 and r % 2:
            t.add('odd_r')
        if r == 1:
            t.add('r1')
        if mode != 'coarse':
            t.add('ncol01' if r <= 2 else 'umulhi')
        if nc == 2:
            t.add('nc2')
        if mode in ('bwd_duc', 'bwd_both'):
            t.add('duc')
        if self.input_kappa:
            t.add('kappa')
        if self.family in ('lane4', 'lane8') and N % 64:
            t.add('ragged_wave')
        if self.family == 'coarse16' and N % 2:
            t.add('ragged_wave')
        if uses_mu:
            t.add('rows_r')
            if r >= 2:
                t.add('backslash')
        if mode == 'bwd_both':
            t.add('no_duc')
        if opt == 'kappa_tiny':
            t.add('kappa_eps')
        if opt == 'loss_scale':
            t.add('scale_value')
        self.tags = t

    def inputs(self):
        return inputs(self.nc, self.r, self.N, self.opt)

    def evaluate(self, dtype=None, wrong=None):
        """The mode's reference on the case's inputs -> dict of float64 arrays (rom_ref)."""
        import torch
        d = self.inputs()
        kw = dict(input_kappa=self.input_kappa, dtype=dtype or torch.float64, wrong=wrong)
        a = (self.nc, self.r, d['x'], d['F'])
        if self.mode == 'forward':
            return R.forward(*a, **kw)
        if self.mode == 'coarse':
            return {'uc': R.forward(*a, **kw)['uc']}
        if self.mode == 'loglik':
            return R.loglik(*a, d['Y'], d['ls'], loss_scale=self.loss_scale, **kw)
        return R.backward(*a, dmu=None if self.mode == 'bwd_duc' else d['dmu'],
                          duc=None if self.mode == 'bwd_dmu' else d['duc'], **kw)

    def reference(self):
        return _reference(self.index)


@functools.lru_cache(maxsize=None)
def _reference(index):
    return cases()[index].evaluate()


def compare(got, ref):
    """quantity -> error of `got` against `ref`, over the quantities the reference has."""
    errs = {}
    for k, r in ref.items():
        if k == 'L':
            errs[k] = abs(got[k] - r) / abs(r)
        elif k == 'L_rows':
            errs[k] = float(np.max(np.abs(np.asarray(got[k], dtype=np.float64) - r) / np.abs(r)))
        else:
            errs[k] = R.rel_err(got[k], r)
    return errs


def over_bar(errs):
    return {k: e for k, e in errs.items() if not e <= BAR[k]}


NATIVE_SHAPES = tuple((nc, r, N) for nc in (4, 8, 16) for r in (1, 2, 3, 5) for N in (1, 3)) + ((4, 7, 3), (8, 7, 3))
GENERIC_SHAPES = tuple((nc, r, 2) for nc in (2, 3, 6, 7, 11, 15) for r in (1, 3)) + ((2, 2, 2), (15, 2, 2))
COARSE_SHAPES = tuple((nc, 2, N) for nc in (4, 8) for N in (1, 63, 64, 65, 130)) + \
    tuple((16, 2, N) for N in (1, 2, 3)) + ((7, 2, 2),)
OPTION_SHAPE = {'fast4': (4, 3, 3), 'fast8': (8, 3, 3), 'fast16': (16, 3, 3), 'generic': (7, 3, 2)}
CONTRAST_SHAPE = {'fast4': (4, 2, 5), 'fast8': (8, 2, 5), 'fast16': (16, 2, 5), 'generic': (7, 2, 5)}
COARSE_NC = {'lane4': 4, 'lane8': 8, 'coarse16': 16, 'generic': 7}


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    add = lambda *a: out.append(Case(len(out), *a))
    for shape in NATIVE_SHAPES + GENERIC_SHAPES:
        for mode in MODES:
            add(*shape, mode)
    for shape in COARSE_SHAPES:
        add(*shape, 'coarse')
    for fam in FULL_FAMILIES:
        for opt in OPTIONS:
            shape = CONTRAST_SHAPE[fam] if opt == 'contrast' else OPTION_SHAPE[fam]
            for mode in OPTION_MODES[opt]:
                add(*shape, mode, opt)
    for fam, nc in COARSE_NC.items():
        for opt in COARSE_OPTIONS:
            add(nc, 2, 5 if opt == 'contrast' else 3, 'coarse', opt)
    return tuple(out)


def select(family=None, mode=None, nc=None):
    return [c for c in cases() if (family is None or c.family == family) and (mode is None or c.mode == mode) and
            (nc is None or c.nc in nc)]


# ---------------------------------------------------------------------- the launch
def rom_desc(nc, r, n, mode, **kw):
    """gpi_rom through its descriptor (every field reachable, unlike gpi.engine.rom_call); tensors by address.
    Returns the return code unless check (default): then a refusal raises."""
    import ctypes as C
    import torch
    from gpi import _lib as L
    check = kw.pop('check', True)
    d = L.RomDesc()
    d.nc, d.refine, d.n, d.mode = nc, r, n, mode
    keep = []
    for k, v in kw.items():
        if torch.is_tensor(v):
            keep.append(v)
            v = v.data_ptr()
        setattr(d, k, v)
    rc = L.lib().gpi_rom(C.byref(d), L.stream_handle())
    torch.cuda.synchronize()
    if check:
        L.check(rc, 'rom')
    return rc
