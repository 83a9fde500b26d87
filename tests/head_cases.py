"""Case table and layout builder of the dense-head operator sweep (tests/test_head_cases_plan.py on the CPU,
tests/test_gpu_head_ops.py on the GPU).  Imports without a GPU.

A case is (layout, counts, mode): the parameter vector, the workspace, and the HeadDesc / GemmItem arrays are
built directly, without a model.  Every workspace region and every parameter block is followed by >= 8 floats of a
fixed NaN bit pattern (GUARD_BITS), and so is every workspace row that is no input of the mode: whatever a launch
must not write still holds the pattern afterwards, bit for bit.

Layouts (d_feat / d_z / d_lat / d_x -> the kernel form default dispatch picks, gpi_head_form):
    80/64/64/128     2  prefetched MFMA
    64/16/64/32      3  prefetched MFMA
    36/20/24/44      1  generic MFMA off the 16-grid; VALU: matvec_t2's row-split path
    96/48/80/160     1  generic MFMA, K > 64: a second c0 pass of contract<>
    256/128/256/256  1  generic MFMA at the MW / MZ limits; VALU: matvec_t2's strided path
    30/10/18/22      0  not multiples of 4: VALU, scalar matvec2
    80/64/64/512     0  the nc = 16 width (d_x > MW)
    36/20/24/44 with gp_w at an offset = 2 mod 4:  0 by the alignment gate (1 where no segment has the gp term)
Counts (n_enc, n_q, n_q2): (16,16,0) (17,5,0) (33,3,14) (0,20,7) (5,0,0) (0,0,9) (1,1,1), and (33,0,0) for the two
stand-alone modes (they need n_q = n_q2 = 0, which leaves them (5,0,0) of the list alone: one more count gives them
several tiles with a partial last one).
Modes: freeX (both segments with the gp term), holdoff (segment 2 without it), lockX, nonamortised (REPARAM
without ENC), enc_engine (ENC alone), dec_engine (LATENT alone).  Dropped combinations: holdoff without a second
segment (3 counts), lockX without variational samples ((5,0,0): the same launch as freeX), nonamortised without
encoder samples (2 counts), the stand-alone modes with variational samples.  That leaves 7 + 4 + 6 + 5 + 2 + 2 = 26
cases per layout, 8 layouts: 208 cases.

Values: O(1) from a fixed seed, logsigmas (parameters and inputs) in [-1.5, 0.5], five different scales none of
which is 1.  The builder walks seeds until the fp64 pre-activations keep min|hpre| >= RELU_MARGIN, so that no ReLU
decision of an fp32 kernel can differ from the reference's and no entry is ever excluded from a comparison.
"""
import functools
import itertools

import numpy as np

import head_ref as R
from head_ref import ENC, REPARAM, QZ, LATENT, GP, LOCKX

GUARD_BITS = 0x7FC5A5A5          # a quiet NaN no kernel produces
GUARD = np.array([GUARD_BITS], dtype=np.uint32).view(np.float32)[0]
NG = 8                           # guard floats after every region / block
RELU_MARGIN = 1e-3
REPLICAS = 16                    # GPI_REPLICAS of the library build (gpi/_lib.py checks it at load)
TS = 16                          # samples per MFMA tile

# the operator bars (max|d| / max|ref|): outputs and terms, gradients
BAR = {'out': 1e-5, 'terms': 1e-5, 'grad': 5e-5}

# name: (widths, gp_w offset mod 4, form by default dispatch)
LAYOUTS = {
    'w80_64_64_128': ((80, 64, 64, 128), 0, 2),
    'w64_16_64_32': ((64, 16, 64, 32), 0, 3),
    'w36_20_24_44': ((36, 20, 24, 44), 0, 1),
    'w96_48_80_160': ((96, 48, 80, 160), 0, 1),
    'w256_128_256_256': ((256, 128, 256, 256), 0, 1),
    'w30_10_18_22': ((30, 10, 18, 22), 0, 0),
    'w80_64_64_512': ((80, 64, 64, 512), 0, 0),
    'w36_20_24_44_gpw2': ((36, 20, 24, 44), 2, 0),
}
FAMILY_LAYOUTS = ('w80_64_64_128', 'w64_16_64_32')
COUNTS = ((16, 16, 0), (17, 5, 0), (33, 3, 14), (0, 20, 7), (5, 0, 0), (0, 0, 9), (1, 1, 1))
ALONE_COUNTS = ((5, 0, 0), (33, 0, 0))
MODES = ('freeX', 'holdoff', 'lockX', 'nonamortised', 'enc_engine', 'dec_engine')
SCALES = {'kl_enc': 1 / 7, 'kl_q': 1 / 3, 'lx': 1 / 5, 'kl_q2': 1 / 11, 'lx2': 1 / 13}


def mode_counts(mode):
    if mode in ('enc_engine', 'dec_engine'):
        return ALONE_COUNTS
    keep = {'freeX': lambda e, q, v: True,
            'holdoff': lambda e, q, v: v > 0,
            'lockX': lambda e, q, v: q + v > 0,
            'nonamortised': lambda e, q, v: e > 0}[mode]
    return tuple(c for c in COUNTS if keep(*c))


def mode_flags(mode, n_enc, n_q, n_q2):
    """(flags, flags2): a segment's flags are set when it has samples, as the engines do."""
    if mode == 'enc_engine':
        return ENC, 0
    if mode == 'dec_engine':
        return LATENT, 0
    gpf = GP | (LOCKX if mode == 'lockX' else 0)
    f1 = LATENT
    if n_enc:
        f1 |= REPARAM | (0 if mode == 'nonamortised' else ENC)
    if n_q:
        f1 |= QZ | gpf
    f2 = (QZ | (0 if mode == 'holdoff' else gpf)) if n_q2 else 0
    return f1, f2


class Region:
    def __init__(self, off, shape):
        self.off, self.shape = off, shape
        self.size = int(np.prod(shape))

    def view(self, flat):
        return flat[self.off:self.off + self.size].reshape(self.shape)


def _layout(shapes, pad_before=None):
    """Regions in order, each at a multiple of 4 floats (plus pad_before[name]), NG guard floats after each."""
    regs, off = {}, NG
    for name, shape in shapes:
        off = (off + 3) & ~3
        off += (pad_before or {}).get(name, 0)
        regs[name] = Region(off, shape)
        off += max(int(np.prod(shape)), 1) + NG
    return regs, (off + 3) & ~3


class Case:
    def __init__(self, index, layout, counts, mode):
        self.index, self.layout, self.counts, self.mode = index, layout, counts, mode
        self.widths, gpw_mod, self.form = LAYOUTS[layout]
        self.n_enc, self.n_q, self.n_q2 = counts
        self.id = '%s-%d_%d_%d-%s' % ((layout,) + counts + (mode,))
        self.flags, self.flags2 = mode_flags(mode, *counts)
        if gpw_mod and not ((self.flags | self.flags2) & GP):
            self.form = 1                                  # no gp term: gp_w is not read, its offset not gated
        self.scales = dict(SCALES)
        ne, nq, nq2 = counts
        B, nqt = ne + nq + nq2, nq + nq2
        df, dz, dl, dx = self.widths
        self.p_reg, self.n_params = _layout(
            [('fc_w', (df, df)), ('fc_b', (df,)), ('mu_w', (dz, df)), ('mu_b', (dz,)), ('ls_w', (dz, df)),
             ('ls_b', (dz,)), ('lat_w', (dl, dz)), ('lat_b', (dl,)), ('gp_w', (dx, dz)), ('gp_b', (dx,)),
             ('gp_ls', (dx,)), ('qz_mu', (nq, dz)), ('qz_ls', (nq, dz)), ('qx_mu', (nq, dx)), ('qx_ls', (nq, dx)),
             ('qz_mu2', (nq2, dz)), ('qz_ls2', (nq2, dz)), ('qx_mu2', (nq2, dx)), ('qx_ls2', (nq2, dx))],
            {'gp_w': gpw_mod})
        self.w_reg, self.n_ws = _layout(
            [(k, (ne, df)) for k in ('feat', 'gfeat', 'hpre', 'dhpre')] +
            [(k, (B, dz)) for k in ('zmu', 'zls', 'eps_z', 'z', 'gz', 'dzmu', 'dzls')] +
            [(k, (B, dl)) for k in ('lat', 'glat')] +
            [(k, (nqt, dx)) for k in ('eps_x', 'xs', 'mux', 'gxs', 'gmux')])
        self._draw()
        # tile structure (TS samples per tile; encoder and variational samples in separate tiles)
        et = (ne + TS - 1) // TS
        self.partial_enc_after_full = ne > TS and ne % TS != 0
        self.partial = ne % TS != 0 or nqt % TS != 0
        self.drop_sample = ne - 1 if ne % TS else B - 1
        # index of the tile that holds samples of both segments (segment 1 ends inside it), or -1
        self.mixed_tile = et + nq // TS if (nq % TS and nq2) else -1
        f1, f2 = self.flags, self.flags2
        self.tags = set()
        if nq2 and (f2 & QZ):
            self.tags.add('seg2_scales')
        if nq and nq2:
            self.tags.add('seg2_rows')
        if self.partial:
            self.tags.add('drop_last')
        if ne and (f1 & ENC):
            self.tags.add('no_relu_mask')
        if (nq and (f1 & GP) and not (f1 & LOCKX)) or (nq2 and (f2 & GP) and not (f2 & LOCKX)):
            self.tags.add('no_entropy')
        if mode == 'holdoff':
            self.tags.add('holdoff_gp')

    # ------------------------------------------------------------------ values
    def _draw(self):
        ne, nq, nq2 = self.counts
        B, nqt = ne + nq + nq2, nq + nq2
        df, dz, dl, dx = self.widths
        for attempt in itertools.count():
            rng = np.random.default_rng(7919 * self.index + 104729 * attempt + 17)
            n32 = lambda *s: rng.standard_normal(s).astype(np.float32)
            ls32 = lambda *s: rng.uniform(-1.5, 0.5, s).astype(np.float32)
            fc_w, fc_b, feat = (4.0 / np.sqrt(df)) * n32(df, df), n32(df), n32(ne, df)
            hpre = feat.astype(np.float64) @ fc_w.astype(np.float64).T + fc_b.astype(np.float64)
            if hpre.size == 0 or np.abs(hpre).min() >= 1.001 * RELU_MARGIN:
                break
            assert attempt < 10000
        self.seed_attempts = attempt + 1
        self.params = {
            'fc_w': fc_w, 'fc_b': fc_b,
            'mu_w': (0.5 / np.sqrt(df)) * n32(dz, df), 'mu_b': 0.5 * n32(dz),
            'ls_w': (0.05 / np.sqrt(df)) * n32(dz, df), 'ls_b': rng.uniform(-0.8, -0.2, dz).astype(np.float32),
            'lat_w': n32(dl, dz) / np.sqrt(dz), 'lat_b': n32(dl),
            'gp_w': n32(dx, dz) / np.sqrt(dz), 'gp_b': n32(dx), 'gp_ls': ls32(dx),
            'qz_mu': n32(nq, dz), 'qz_ls': ls32(nq, dz), 'qx_mu': n32(nq, dx), 'qx_ls': ls32(nq, dx),
            'qz_mu2': n32(nq2, dz), 'qz_ls2': ls32(nq2, dz), 'qx_mu2': n32(nq2, dx), 'qx_ls2': ls32(nq2, dx)}
        self.params = {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in self.params.items()}
        self.inputs = {'feat': feat, 'zmu': n32(B, dz), 'zls': ls32(B, dz), 'eps_z': n32(B, dz), 'z': n32(B, dz),
                       'gz': n32(B, dz), 'dzls': n32(B, dz), 'glat': n32(B, dl), 'eps_x': n32(nqt, dx),
                       'gxs': n32(nqt, dx)}

    def input_rows(self):
        """name -> boolean row mask: the workspace rows the mode reads as inputs (everything else starts as the
        guard pattern)."""
        ne, nq, nq2 = self.counts
        B, nqt = ne + nq + nq2, nq + nq2
        f1, f2 = self.flags, self.flags2
        rows = lambda n, *spans: np.isin(np.arange(n), np.concatenate([np.arange(a, b) for a, b in spans] or [[]]))
        enc, s1, s2 = (0, ne), (ne, ne + nq), (ne + nq, B)
        draw = [enc] * bool(f1 & REPARAM) + [s1] * bool(f1 & QZ) + [s2] * bool(f2 & QZ)
        gp = [(0, nq)] * bool(f1 & GP) + [(nq, nqt)] * bool(f2 & GP)
        qx = [(0, nq)] * bool((f1 & GP) and not (f1 & LOCKX)) + [(nq, nqt)] * bool((f2 & GP) and not (f2 & LOCKX))
        m = {'feat': rows(ne, *[enc] * bool(f1 & ENC)),
             'zmu': rows(B, *[enc] * (not f1 & ENC)), 'zls': rows(B, *[enc] * (not f1 & ENC)),
             'eps_z': rows(B, *draw),
             'z': ~rows(B, *draw),
             'gz': rows(B, *[(0, B)] * (not f1 & LATENT)),
             'glat': rows(B, *[(0, B)] * bool(f1 & LATENT)),
             'dzls': rows(B, *[enc] * (not f1 & REPARAM)),
             'eps_x': rows(nqt, *qx), 'gxs': rows(nqt, *gp)}
        return m

    # ------------------------------------------------------------------ flat arrays
    def param_vector(self):
        P = np.full(self.n_params, GUARD, dtype=np.float32)
        for k, r in self.p_reg.items():
            r.view(P)[...] = self.params[k]
        return P

    def workspace(self):
        ws = np.full(self.n_ws, GUARD, dtype=np.float32)
        for k, m in self.input_rows().items():
            self.w_reg[k].view(ws)[m] = self.inputs[k][m]
        return ws

    def param_mask(self):
        m = np.zeros(self.n_params, dtype=bool)
        for r in self.p_reg.values():
            m[r.off:r.off + r.size] = True
        return m

    def desc(self, L, terms_ptr, extra_flags=0):
        """The gpi_head_desc (L: gpi._lib).  terms_ptr: address of (4 + 3) * REPLICAS doubles."""
        h = L.HeadDesc()
        h.flags, h.flags2 = self.flags | extra_flags, self.flags2
        h.n_enc, h.n_q, h.n_q2 = self.counts
        h.d_feat, h.d_z, h.d_lat, h.d_x = self.widths
        for k, r in self.p_reg.items():
            setattr(h, k, r.off)
        for k, r in self.w_reg.items():
            setattr(h, k, r.off)
        s = self.scales
        h.kl_scale_enc, h.kl_scale_q, h.lx_scale = s['kl_enc'], s['kl_q'], s['lx']
        h.kl_scale_q2, h.lx_scale2 = s['kl_q2'], s['lx2']
        h.terms = terms_ptr
        h.terms2 = terms_ptr + 4 * REPLICAS * 8
        return h

    def gemm_items(self, L, valu=False):
        """The shared-weight gradients as gpi_outer_gemm items: sum over samples of delta (x) layer input."""
        ne, nq, nq2 = self.counts
        B = ne + nq + nq2
        df, dz, dl, dx = self.widths
        f1, f2 = self.flags, self.flags2
        w, p = self.w_reg, self.p_reg
        its = []

        def item(a, b, S, M, N, c, bias, relu=0):
            its.append(L.GemmItem(a_off=a, b_off=b, c_off=p[c].off, bias_off=p[bias].off, S=S, M=M, N=N, lda=M,
                                  ldb=N, flags=relu))

        if f1 & LATENT:
            item(w['glat'].off, w['z'].off, B, dl, dz, 'lat_w', 'lat_b')
        n_gp = (nq if f1 & GP else 0) + (nq2 if f2 & GP else 0)      # the gp rows are the leading variational ones
        if n_gp:
            item(w['gmux'].off, w['z'].off + ne * dz, n_gp, dx, dz, 'gp_w', 'gp_b')
        if ne and (f1 & ENC):
            item(w['dzmu'].off, w['hpre'].off, ne, dz, df, 'mu_w', 'mu_b', 1)
            item(w['dzls'].off, w['hpre'].off, ne, dz, df, 'ls_w', 'ls_b', 1)
            item(w['dhpre'].off, w['feat'].off, ne, df, df, 'fc_w', 'fc_b')
        if valu and its:
            its[0].flags |= 2
        return (L.GemmItem * len(its))(*its)

    def reference(self):
        return _reference(self.index)

    def extract(self, ws, terms, gacc):
        """A launch's results in the reference's form: ws / gacc flat arrays, terms the (4 + 3) * REPLICAS sums."""
        got = {k: self.w_reg[k].view(ws) for k in R.FWD_REGIONS + R.BWD_REGIONS}
        got['terms'] = np.asarray(terms, dtype=np.float64)[:7 * REPLICAS].reshape(7, REPLICAS).sum(1)
        for k, r in self.p_reg.items():
            got['grad:' + k] = r.view(gacc)
        return got


def region_class(key):
    return 'terms' if key.startswith('terms') else ('out' if key in R.FWD_REGIONS else 'grad')


def compare(got, ref, same_rows=False):
    """key -> error of `got` against `ref` (head_ref.rel_err; each of the seven terms on its own)."""
    errs = {}
    for k, r in ref.items():
        if k == 'terms':
            for i, name in enumerate(R.TERMS):
                errs['terms:' + name] = R.rel_err(got[k][i:i + 1], r[i:i + 1])
        else:
            errs[k] = R.rel_err(got[k], r, same_rows)
    return errs


def worst(errs):
    """class -> (max error, key)"""
    w = {}
    for k, e in errs.items():
        c = region_class(k)
        if c not in w or e > w[c][0]:
            w[c] = (e, k)
    return w


def over_bar(errs):
    return {k: e for k, e in errs.items() if e > BAR[region_class(k)]}


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for layout in LAYOUTS:
        for mode in MODES:
            for counts in mode_counts(mode):
                out.append(Case(len(out), layout, counts, mode))
    return tuple(out)


def layout_cases(layout):
    return [c for c in cases() if c.layout == layout]


@functools.lru_cache(maxsize=None)
def _reference(index):
    return R.head_reference(cases()[index])


# ---------------------------------------------------------------------- bare gpi_outer_gemm cases
GEMM_S = (1, 3, 17, 67, 130)
GEMM_MN = ((16, 16), (20, 36), (5, 1), (44, 20))


class GemmCase:
    """One gpi_outer_gemm launch: items (dicts, head_ref.gemm_reference), the workspace and the accumulator layout.
    Rows are strided (lda = M + 3, ldb = N + 1) so a read past a row's width lands in another row, not in a
    guard."""

    def __init__(self, index, specs):
        rng = np.random.default_rng(1009 * index + 5)
        self.id = '+'.join('S%d_M%d_N%d_b%d_r%d' % s for s in specs)
        shapes, gshapes = [], []
        for k, (S, M, N, bias, relu) in enumerate(specs):
            shapes += [('a%d' % k, (S, M + 3)), ('b%d' % k, (S, N + 1))]
            gshapes += [('c%d' % k, (M, N)), ('bias%d' % k, (M,))]
        self.w_reg, self.n_ws = _layout(shapes)
        self.g_reg, self.n_gacc = _layout(gshapes)
        self.ws = np.full(self.n_ws, GUARD, dtype=np.float32)
        self.items = []
        for k, (S, M, N, bias, relu) in enumerate(specs):
            for nm in ('a%d' % k, 'b%d' % k):
                r = self.w_reg[nm]
                r.view(self.ws)[...] = rng.standard_normal(r.shape).astype(np.float32)
            self.items.append(dict(a_off=self.w_reg['a%d' % k].off, b_off=self.w_reg['b%d' % k].off, S=S, M=M, N=N,
                                   lda=M + 3, ldb=N + 1, relu=relu, bias=bias, c_off=self.g_reg['c%d' % k].off,
                                   bias_off=self.g_reg['bias%d' % k].off if bias else -1))

    def gemm_items(self, L, valu):
        its = [L.GemmItem(a_off=i['a_off'], b_off=i['b_off'], c_off=i['c_off'], bias_off=i['bias_off'], S=i['S'],
                          M=i['M'], N=i['N'], lda=i['lda'], ldb=i['ldb'], flags=int(i['relu'])) for i in self.items]
        if valu:
            its[0].flags |= 2
        return (L.GemmItem * len(its))(*its)

    def reference(self):
        """The whole accumulator in fp64: C and bias blocks, zero elsewhere."""
        g = np.zeros(self.n_gacc)
        for k, (c, b) in enumerate(R.gemm_reference(self.items, self.ws)):
            self.g_reg['c%d' % k].view(g)[...] = c
            if b is not None:
                self.g_reg['bias%d' % k].view(g)[...] = b
        return g


@functools.lru_cache(maxsize=None)
def gemm_cases():
    out = []
    for S in GEMM_S:
        for M, N in GEMM_MN:
            for bias in (1, 0):
                for relu in (0, 1):
                    out.append(GemmCase(len(out), [(S, M, N, bias, relu)]))
    out.append(GemmCase(len(out), [(67, 20, 36, 1, 1), (3, 16, 16, 0, 0), (130, 5, 1, 1, 0), (17, 44, 20, 0, 1)]))
    return tuple(out)
