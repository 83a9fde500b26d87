"""Test-only case table of the per-operator conv sweep (no test functions).

Each case is one tiny synthetic CodecProgram around ONE conv under test, T, chosen so that conv.hip's
host planner (conv_geom / launch / select_kernel / cp_of / lsum_op / vsum_op) sends T's launches down a
combination of kernel variants the shipped configurations never reach.  tests/test_conv_cases_plan.py
proves on the host that the table reaches every variant (and none of the compile-time shape kernels);
tests/test_gpu_conv_ops.py runs every case on the GPU against the fp64 interpreter
(tests/program_interp.py).

The program around T (chain()):
  producers  1x1 convs without BN from a 4-channel internal input buffer 'z' into T's cin input channels,
             one per 8 channels (cout <= GPI_MAX_COUT): T's backward writes an input gradient, the producers'
             backward runs gout_mode 0 on the S buffer and the BN-backward sums T wrote;
  T          input BN + ReLU, the geometry under test, statistics epilogue;
  consumer   1x1 conv with input BN to a 3-channel output buffer (gout_mode 1), so T's own backward runs
             gout_mode 0.
dense: T reads channels [0, cin) and writes [cin, cin + cout) of one buffer the consumer reads whole
(plan.py _dense_layer: gin_accumulate 1).  ext: T is the 7x7 stride-2 conv on the external one-channel
input (no producers, no input BN).  loss: T is the 5x5 output conv with a Gaussian-loss epilogue, no
consumer.  drop: Dropout2d scales on T.  T's output buffer carries one spare channel no op writes.
"""
import ctypes as C
import os
import re

from gpi import _lib as L
from gpi.engine import Workspace, groups_struct
from gpi.plan import Arena, CodecProgram

CONV_HIP = os.path.join(L.SRC_DIR, 'conv.hip')
CONV_SHAPES_H = os.path.join(L.SRC_DIR, 'conv_shapes.h')
DROP_P = 0.25


class Case(object):
    def __init__(self, k, mode, cin, cout, h, w, groups, dense=False, ext=False, loss=None, drop=False,
                 grad=True, shuffle=False, loss_scale=None, seed=0, reach=None, bars=None):
        """mode: 's1' | 's2' | 'up'; (h, w): T's input plane; groups: BN group sizes; loss: None | 'gauss' |
        'exp'; shuffle: ext rows a shuffled ext_idx, loss rows a shuffled tgt_idx on group 0;
        reach: {'fwd' | 'bwd' | 'fuse': {shape field: value}} the variants the planner must report for T;
        bars: {check: bar} overrides of the project bars, each with both measured numbers next to it."""
        self.k, self.mode, self.cin, self.cout, self.h, self.w = k, mode, cin, cout, h, w
        self.groups = list(groups)
        self.dense, self.ext, self.loss, self.drop, self.grad = dense, ext, loss, drop, grad
        self.shuffle, self.loss_scale, self.seed = shuffle, loss_scale, seed
        self.reach = reach or {}
        self.bars = bars or {}

    @property
    def B(self):
        return sum(self.groups)

    @property
    def out_plane(self):
        if self.mode == 's2':
            return self.h // 2, self.w // 2
        if self.mode == 'up':
            return 2 * self.h, 2 * self.w
        return self.h, self.w

    @property
    def id(self):
        tag = 'k%d%s_%dto%d_%dx%d_g%s' % (self.k, self.mode, self.cin, self.cout, self.h, self.w,
                                          '+'.join(str(n) for n in self.groups))
        for flag, name in ((self.dense, 'dense'), (self.ext, 'ext'), (self.loss, self.loss), (self.drop, 'drop'),
                           (self.shuffle, 'shuf'), (not self.grad, 'fwdonly')):
            if flag:
                tag += '_' + name
        return tag


def R(fwd=None, bwd=None, fuse=None):
    return {k: v for k, v in (('fwd', fwd), ('bwd', bwd), ('fuse', fuse)) if v is not None}


# T (k, stride/up, cin, cout, input plane), BN groups, and what the planner must report for it
# (npxk 0 = the channel-group instantiation)
CASES = [
    # --- 3x3 stride 1
    Case(3, 's1', 6, 4, 8, 8, [3, 2], seed=1,
         reach=R(dict(cg=4, cp=4, npxk=0), dict(zreg=1, lsum=1, split=1))),
    Case(3, 's1', 3, 8, 4, 4, [4], seed=2, reach=R(dict(cg=3, cp=8), dict(lsum=1))),
    Case(3, 's1', 8, 4, 16, 16, [130], dense=True, seed=3,
         reach=R(None, dict(half=1, lsum=1, split=1, D_gin_accumulate=1))),
    Case(3, 's1', 12, 4, 16, 16, [256, 128], dense=True, seed=4,
         reach=R(dict(half=1), dict(half=0, split=0))),
    Case(3, 's1', 4, 4, 16, 16, [260], seed=5, reach=R(dict(half=1), dict(half=1, lsum=1, split=0))),
    Case(3, 's1', 16, 8, 32, 32, [2, 1], seed=6, reach=R(None, dict(zreg=0))),
    Case(3, 's1', 10, 5, 32, 32, [2], seed=7, reach=R(dict(cp=8, G_th=8))),
    Case(3, 's1', 8, 4, 32, 32, [2], seed=8, reach=R(None, dict(G_th=16))),
    Case(3, 's1', 4, 4, 64, 64, [2], seed=9, reach=R(dict(npxk=4))),
    Case(3, 's1', 12, 4, 64, 64, [2], seed=10, reach=R(dict(G_th=4))),
    Case(3, 's1', 4, 4, 24, 20, [2], seed=11, reach=R(None, dict(G_tiles=3))),
    Case(3, 's1', 4, 4, 256, 256, [1], seed=12, reach=R(None, dict(G_tiles=128, G_th=2))),
    # --- 1x1
    Case(1, 's1', 5, 5, 8, 8, [260], seed=13, reach=R(dict(cp=6, cg=4), dict(half=1, lsum=1))),
    Case(1, 's1', 14, 7, 16, 16, [3], seed=14, reach=R(dict(cp=8), dict(lsum=1))),
    Case(1, 's1', 16, 8, 64, 64, [2], seed=15, reach=R(None, dict(zreg=0))),
    Case(1, 's1', 9, 1, 32, 32, [2], seed=16, reach=R(dict(cp=2))),
    # --- 3x3 stride 2
    Case(3, 's2', 5, 5, 32, 32, [2], seed=17, reach=R(dict(cp=6, cg=2), dict(lsum=1, split=1))),
    Case(3, 's2', 8, 8, 16, 16, [3], seed=18, reach=R(dict(cg=4, cp=8))),
    Case(3, 's2', 3, 3, 8, 8, [2], seed=19, reach=R(dict(cg=3))),
    Case(3, 's2', 10, 5, 16, 16, [300], seed=20, reach=R(None, dict(half=1, lsum=1, split=0))),
    Case(3, 's2', 16, 8, 64, 64, [2], seed=21, reach=R(dict(cg=2, cp=8))),
    Case(3, 's2', 6, 6, 128, 128, [1], seed=22, reach=R(dict(G_tiles=32, G_th=2))),
    # (24 x 48, not 24 x 40: on the 12 x 20 output plane the 1x1 consumer's backward is itself refused -- six owned
    # rows of 20 pixels are no whole number of 16-pixel column blocks; same variants: non-square, 3 backward tiles)
    Case(3, 's2', 4, 4, 24, 48, [2], seed=23, reach=R(dict(G_tiles=3), dict(G_tiles=3))),
    # --- 3x3 on the nearest x2 upsampled input
    Case(3, 'up', 6, 6, 8, 8, [3], seed=24, reach=R(dict(cp=6), dict(ucls=1, lsum=1))),
    Case(3, 'up', 5, 3, 16, 16, [2], seed=25, reach=R(dict(npxk=2), dict(ucls=0))),
    Case(3, 'up', 8, 4, 32, 32, [2], seed=26, reach=R(dict(npxk=4), dict(ucls=1, zreg=0))),
    Case(3, 'up', 11, 2, 4, 4, [2], seed=27, reach=R(None, dict(ucls=1))),
    Case(3, 'up', 16, 8, 16, 16, [2], seed=28, reach=R(None, dict(ucls=1, zreg=0))),
    Case(3, 'up', 3, 3, 128, 128, [1], seed=29, reach=R(dict(D_w_out=256))),
    # --- 7x7 stride 2 on the external one-channel input
    Case(7, 's2', 1, 6, 32, 32, [3], ext=True, seed=30, reach=R(dict(cp=8), dict(vshift=1, vsum=1))),
    Case(7, 's2', 1, 6, 32, 32, [3], ext=True, shuffle=True, seed=31, reach=R(None, dict(vshift=1, vsum=1))),
    Case(7, 's2', 1, 8, 64, 64, [2], ext=True, shuffle=True, seed=32, reach=R(dict(npxk=2), dict(zreg=0))),
    Case(7, 's2', 1, 4, 16, 16, [2], ext=True, seed=33, reach=R(None, dict(vshift=1, vsum=0))),
    # --- 5x5 output conv with the Gaussian-loss epilogue (separate launches and fused)
    Case(5, 's1', 3, 2, 16, 16, [2, 1], loss='gauss', seed=34, reach=R(None, dict(half=0), dict(half=0))),
    Case(5, 's1', 1, 2, 8, 8, [2], loss='gauss', seed=35),
    Case(5, 's1', 4, 2, 32, 32, [32, 8], loss='gauss', seed=36, reach=R(dict(G_th=8), dict(G_th=32))),
    Case(5, 's1', 4, 2, 64, 64, [64, 8], loss='exp', shuffle=True, loss_scale=[0.5, 1.0 / 8], seed=37,
         reach=R(dict(half=1), dict(half=1), dict(half=1))),
    # --- forward only: cin above the backward limit
    Case(3, 's1', 17, 8, 8, 8, [2], grad=False, seed=38, reach=R(dict(cg=4))),
    Case(3, 's1', 32, 8, 8, 8, [2], grad=False, seed=39, reach=R(dict(cg=4))),
    # --- Dropout2d twins (scales 0 and 1 / (1 - p), one sample with every channel dropped)
    Case(3, 's1', 6, 4, 8, 8, [3, 2], drop=True, seed=40, reach=R(dict(drop=1), dict(drop=1))),
    Case(3, 's2', 8, 8, 16, 16, [3], drop=True, seed=41, reach=R(dict(drop=1, cg=4), dict(drop=1, lsum=1))),
    Case(3, 'up', 6, 6, 8, 8, [3], drop=True, seed=42, reach=R(dict(drop=1), dict(drop=1))),
]

# backward launches the planner must refuse (GPI_ERR_UNSUPPORTED): owned input rows that are no whole
# number of 16-pixel MFMA column blocks, and every backward of more than 16 input channels
REFUSALS = [
    Case(3, 's1', 4, 4, 12, 12, [2], seed=50),
    Case(3, 'up', 4, 4, 6, 12, [2], seed=51),
    Case(3, 's1', 17, 8, 8, 8, [2], seed=52),
    Case(1, 's1', 20, 4, 16, 16, [2], seed=53),
]


def chain(case):
    """The CodecProgram of a case; prog.T is the op under test."""
    P = CodecProgram('conv_case', DROP_P if case.drop else 0.0)
    h, w = case.h, case.w
    oh, ow = case.out_plane
    pad = case.k // 2
    stride = 2 if case.mode == 's2' else 1
    up = 1 if case.mode == 'up' else 0
    epi = {None: None, 'gauss': L.EPI_GAUSS_LOSS, 'exp': L.EPI_GAUSS_EXP_LOSS}[case.loss]
    if case.ext:
        assert case.k == 7 and case.mode == 's2' and case.cin == 1
        x = P.buf('input', 1, h, w)
        x.external = True
        P.input = x
        Y = P.buf('Y', case.cout + 1, oh, ow)
        P.T = P.conv('T', x, 0, 1, Y, 0, case.cout, 7, 2, 3, 0, 'T.weight', dropout=case.drop)
    else:
        z = P.buf('z', 4, h, w)
        P.input = z
        if case.dense:
            assert case.mode == 's1' and not case.loss
            X = P.buf('X', case.cin + case.cout + 1, h, w)
            Y, d0 = X, case.cin
        elif case.loss:
            X = P.buf('X', case.cin, h, w)
            Y, d0 = P.buf('out', 2, oh, ow), 0
        else:
            X = P.buf('X', case.cin, h, w)
            Y, d0 = P.buf('Y', case.cout + 1, oh, ow), 0
        for i, c0 in enumerate(range(0, case.cin, L.GPI_MAX_COUT)):
            n = min(L.GPI_MAX_COUT, case.cin - c0)
            P.conv('p%d' % i, z, 0, 4, X, c0, n, 1, 1, 0, 0, 'p%d.weight' % i)
        P.T = P.conv('T', X, 0, case.cin, Y, d0, case.cout, case.k, stride, pad, up, 'T.weight', bn='T.bn',
                     epilogue=epi, dropout=case.drop)
    if case.loss:
        P.output = Y
    else:
        nread = case.cin + case.cout if case.dense else case.cout
        out = P.buf('out', 3, oh, ow)
        P.conv('c', Y, 0, nread, out, 0, 3, 1, 1, 0, 0, 'c.weight', bn='c.bn')
        P.output = out
    return P


def param_shapes(prog):
    """[(name, shape)] of the program's parameters: each conv's weight, then its input BN's gamma and beta
    (adjacent, so the two reduce as one slab item)."""
    out = []
    for op in prog.ops:
        out.append((op.w, (op.cout, op.cin, op.k, op.k)))
        if op.bn is not None:
            out += [(op.bn + '.weight', (op.cin,)), (op.bn + '.bias', (op.cin,))]
    return out


class RecordingArena(Arena):
    """Arena that remembers its allocations [(offset, elements)]."""

    def __init__(self, align=64):
        Arena.__init__(self, align)
        self.allocs = []

    def alloc(self, n):
        off = Arena.alloc(self, n)
        self.allocs.append((off, int(n)))
        return off


def lay_out(case, prog, param_offset=None):
    """(workspace, gpi_groups, descriptors) of the program at the case's batch, as the engines lay theirs out."""
    ws = Workspace()
    ws.ws = RecordingArena()
    g = groups_struct(case.groups)
    descs = prog.layout(case.B, ws.ws, ws.stats, ws.parts, g, param_offset or (lambda name: 0), grad=case.grad)
    return ws, g, descs


# ------------------------------------------------------------------ shapes (conv.hip ShapeC)
def shape_fields():
    """Names of ShapeC's ints in order, read from conv.hip: the leading variant ints, then D_<n> over SHAPE_D,
    G_<n> over SHAPE_G (what follows -- magic divisors, the half-tile geometry -- is not named here)."""
    src = open(CONV_HIP).read()
    src = src.replace('\\\n', ' ')

    def macro(name):
        m = re.search(r'#define %s\(X\)(.*)' % name, src)
        return re.findall(r'X\((\w+)\)', m.group(1))

    m = re.search(r'struct ShapeC \{.*?\n\s*int ([\w\s,]+);', src, re.S)
    lead = [n.strip() for n in m.group(1).split(',')]
    return lead + ['D_' + n for n in macro('SHAPE_D')] + ['G_' + n for n in macro('SHAPE_G')]


def parse_shapes(text):
    """The integer rows of a GPI_CONV_SHAPE_LIST (conv_shapes.h / gpi_conv_shapes_dump)."""
    return [tuple(int(v) for v in row.split(',')) for row in re.findall(r'\{([-\d,]+)\}', text.split(
        'GPI_CONV_SHAPE_LIST', 1)[1].split('#define', 1)[0])]


def recorded_shapes(lib):
    buf = C.create_string_buffer(1 << 22)
    L.check(lib.gpi_conv_shapes_dump(buf, len(buf)), 'gpi_conv_shapes_dump')
    return parse_shapes(buf.value.decode())


def plan_shape(lib, d, ctx, fwd, fuse, fields=None):
    """(return code, decoded shape or None) of one gpi_conv_shape_plan.  The recording is process-global and
    keeps each distinct shape once (fields None: the return code only): the shape is the entry the call added, or, when an earlier call already
    recorded the same shape, the one recorded entry that agrees with the descriptor."""
    before = recorded_shapes(lib) if fields else None
    rc = lib.gpi_conv_shape_plan(C.byref(d), C.byref(ctx), 1 if fwd else 0, 1 if fuse else 0)
    if rc != 0 or not fields:
        return rc, None
    after = recorded_shapes(lib)
    if len(after) == len(before) + 1:
        row = after[-1]
    else:
        assert len(after) == len(before)
        want = dict(fwd=int(bool(fwd)), fusek=int(bool(fuse)), has_gin=int(d.gin_off >= 0),
                    drop=int(d.drop_off >= 0), wout=int(d.wpart_off >= 0), ext_in=int(d.in_off < 0))
        for n in ('k', 'stride', 'pad', 'upsample', 'cin', 'cout', 'h_in', 'w_in', 'h_out', 'w_out', 'in_bn',
                  'gout_mode', 'epilogue', 'gin_accumulate'):
            want['D_' + n] = getattr(d, n)
        cands = [r for r in after if all(r[fields.index(k)] == v for k, v in want.items())]
        # the same op at another batch can differ in the half-tile fields only; callers plan each distinct
        # (op, batch) once, so more than one candidate means the table holds two such rows
        assert len(cands) == 1, 'ambiguous recorded shape for %r' % want
        row = cands[0]
    s = dict(zip(fields, row))
    s['_row'] = row
    return rc, s


def plan_ctx(g):
    """A codec context good for host planning only (no device call reads its pointers)."""
    ctx = L.CodecCtx()
    ctx.ws = 1 << 12
    ctx.ext_in = 1 << 12
    ctx.ext_stride = 1 << 12
    ctx.groups = g
    return ctx
