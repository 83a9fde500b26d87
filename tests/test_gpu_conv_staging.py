"""Operand staging of the conv kernels through buffer descriptors (conv.hip stage / stage_img): padding is an
out-of-range buffer offset, which the hardware turns into a zero LDS chunk.

  probe      gpi_debug_buffer_lds_probe: in-range lanes of a 16-byte and a 4-byte buffer LDS-DMA load carry their
             data; out-of-range lanes (offset == num_records, past it, and the kernels' padding constant, the most
             negative offset) write ZERO over the LDS sentinel -- the outcome stage / stage_img are built on.
             (Every out-of-range offset used here lies inside the test's own allocation or is out of range under
             every reading of the range rule; -16 is not probed: where the rule were evaluated with 32-bit wrap
             it would be "in range" and address memory 4 GB past the buffer.)
  counts     all-ones input and weights, no BN, no dropout: every output is the integer number of its in-plane
             taps times cin, every input gradient (all-ones output gradient) the number of (output, tap) pairs
             that read the pixel times cout, every weight gradient the number of in-plane positions of its tap:
             exact in fp32, compared with == against an fp64 evaluation.
  poison     the operand planes inside buffers whose other channels (before and after every sample's planes),
             allocation gaps, unused pool / target rows are NaN: every result is finite and bit-identical to the
             run with those neighbours zero.
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from gpi import _lib as L
from gpi.engine import N_TERMS, Workspace, groups_struct, make_ctx, run_reduce
from gpi.flat import FlatParameters
from gpi.plan import CodecProgram

pytestmark = pytest.mark.gpu

SENTINEL = 0xdeadbeef
INT_MIN = -(1 << 31)


# ---------------------------------------------------------------------------------------------- probe
def test_buffer_lds_dma_out_of_range_writes_zero(device):
    lib = L.lib()
    n, margin = 128, 64                       # the window: 512 bytes; 256-byte margins of a telltale value
    buf = torch.full((margin + n + margin,), 777.0, dtype=torch.float32, device=device)
    buf[margin:margin + n] = torch.arange(1, n + 1, dtype=torch.float32, device=device)
    nbytes = 4 * n
    off16 = np.zeros(64, np.int32)
    off4 = np.zeros(64, np.int32)
    in16 = np.zeros(64, bool)
    in4 = np.zeros(64, bool)
    for lane in range(64):
        if lane < 32:                         # every chunk of the window once, in a scrambled order
            off16[lane], in16[lane] = 16 * ((lane * 5) % 32), True
            off4[lane], in4[lane] = 4 * ((lane * 37) % n), True
        elif lane % 2:                        # in range again, among out-of-range lanes
            off16[lane], in16[lane] = 16 * (lane - 32), True
            off4[lane], in4[lane] = nbytes - 4 * (lane - 32), True      # 508 = the last word, downwards
        else:                                 # past the end, inside the right margin
            off16[lane] = nbytes + 16 * ((lane - 32) // 2)
            off4[lane] = nbytes + 4 * ((lane - 32) // 2)
    off16[32] = off4[32] = nbytes             # offset == num_records exactly
    off16[34] = off4[34] = INT_MIN            # the kernels' padding offset (negative)
    in16[[32, 34]] = in4[[32, 34]] = False
    assert (off16 % 16 == 0).all() and (off4 % 4 == 0).all() and nbytes % 16 == 0
    d16 = torch.tensor(off16, device=device)
    d4 = torch.tensor(off4, device=device)
    out = torch.zeros(320, dtype=torch.int32, device=device)
    src_ptr = buf.data_ptr() + 4 * margin
    L.check(lib.gpi_debug_buffer_lds_probe(C.c_void_p(src_ptr), nbytes, C.c_void_p(d16.data_ptr()),
                                           C.c_void_p(d4.data_ptr()), C.c_void_p(out.data_ptr()), L.stream_handle()),
            'probe')
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.float32)
    window = np.arange(1, n + 1, dtype=np.float32)
    want16 = np.zeros((64, 4), np.float32)
    want4 = np.zeros(64, np.float32)
    for lane in range(64):
        if in16[lane]:
            want16[lane] = window[off16[lane] // 4: off16[lane] // 4 + 4]
        if in4[lane]:
            want4[lane] = window[off4[lane] // 4]
    g16, g4 = got[:256].reshape(64, 4), got[256:]
    bits = lambda a: a.view(np.uint32)
    print('out-of-range 16-byte lanes hold', sorted(set(hex(v) for v in bits(g16[~in16]).ravel())),
          '4-byte lanes', sorted(set(hex(v) for v in bits(g4[~in4]))))
    assert (bits(g16[in16]) == bits(want16[in16])).all() and (bits(g4[in4]) == bits(want4[in4])).all()
    assert not (bits(got) == SENTINEL).any(), 'an out-of-range lane left its LDS slot untouched'
    assert (bits(g16[~in16]) == 0).all() and (bits(g4[~in4]) == 0).all()


# ---------------------------------------------------------------------------------------------- runner
def _out_plane(mode, h, w):
    return (h // 2, w // 2) if mode == 's2' else (2 * h, 2 * w) if mode == 'up' else (h, w)


def _run(prog, groups, device, params, fill, x=None, pool=None, ext_idx=None, R=None, targets=None, tgt_idx=None,
         fused=False):
    """Forward, backward and slab reduction of a program on the GPU, every byte of the workspace nobody sets up
    filled with `fill` first.  x: the values of the channels of the input buffer that the first op reads
    (prog.x_c0 on).  Returns {name: numpy array} of every result."""
    lib = L.lib()
    B = sum(groups)
    named = [(n, torch.nn.Parameter(v.clone())) for n, v in params.items()]
    flat = FlatParameters(named, device)
    offset = lambda name: flat.name_offsets[name]
    ws = Workspace()
    descs = prog.layout(B, ws.ws, ws.stats, ws.parts, groups_struct(groups), offset, grad=True)
    ws.materialize(device)
    ws.t_ws.fill_(fill)
    ctx = make_ctx(ws, flat, groups)
    hold = []

    def dev(t):
        t = t.contiguous().to(device)
        hold.append(t)
        return t

    zb = prog.input
    if pool is not None:
        ctx.ext_in = dev(pool).data_ptr()
        ctx.ext_stride = zb.H * zb.W
        if ext_idx is not None:
            ctx.ext_idx = dev(ext_idx).data_ptr()
    else:
        ws.view(zb.off, B, zb.C, zb.H, zb.W)[:, prog.x_c0:prog.x_c0 + x.shape[1]].copy_(x)
    o = prog.output
    if targets is not None:
        for gi in range(len(groups)):
            ctx.tgt[gi] = dev(targets[gi]).data_ptr()
            if tgt_idx[gi] is not None:
                ctx.tgt_idx[gi] = dev(tgt_idx[gi]).data_ptr()
    else:
        ws.view(o.s_off, B, o.C, o.H, o.W)[:, prog.r_c0:prog.r_c0 + R.shape[1]].copy_(R)
    st = L.stream_handle()
    ws.zero_scratch()
    flat.gacc.zero_()
    n_ops = len(descs)
    n_plain = n_ops - 1 if fused else n_ops
    L.check(lib.gpi_codec_forward(descs, n_plain, C.byref(ctx), st), 'forward')
    if fused:
        descs[n_ops - 1].out_off = -1
        L.check(lib.gpi_conv_loss_fused(C.byref(descs[n_ops - 1]), C.byref(ctx), st), 'fused')
    L.check(lib.gpi_codec_backward(descs, n_plain, C.byref(ctx), st), 'backward')
    run_reduce(prog.reduce_items(offset), ws, flat, st)
    torch.cuda.synchronize()
    w = ws.t_ws.cpu().numpy()
    res = {'gacc': flat.gacc.cpu().numpy().copy(), 'offset': offset}
    for op in prog.ops:
        if not (fused and op is prog.ops[-1]):
            b = op.dst
            res['out ' + op.name] = w[b.off:b.off + B * b.per_sample].reshape(B, b.C, b.H, b.W)[
                :, op.d0:op.d0 + op.cout].copy()
        if op.desc.gin_off >= 0:
            b = op.src
            res['gin ' + op.name] = w[b.s_off:b.s_off + B * b.per_sample].reshape(B, b.C, b.H, b.W)[
                :, op.c0:op.c0 + op.cin].copy()
    if targets is not None:
        scr = ws.t_scr.cpu().numpy()
        res['logl'] = scr[:N_TERMS * L.GPI_REPLICAS].copy()
    return res


# ---------------------------------------------------------------------------------------------- exact counts
# (k, mode, cin, cout, h, w): the smallest shapes that reach every staging branch -- halo columns on both
# sides, rows above and below the plane, stride-2 and upsampled row ranges, the 7x7's three-row reach, and on
# 32 x 32 several tiles per sample: a first tile (rows above), a last one (rows below), a half tile
COUNT_CASES = [(3, 's1', 3, 2, 8, 8), (3, 's2', 3, 2, 16, 16), (1, 's1', 3, 2, 8, 8), (3, 'up', 3, 2, 8, 8),
               (7, 's2', 1, 2, 16, 16), (3, 's1', 3, 2, 32, 32)]
GROUPS = [2, 1]


def _count_program(k, mode, cin, cout, h, w):
    P = CodecProgram('staging_counts')
    oh, ow = _out_plane(mode, h, w)
    X = P.buf('X', cin, h, w)
    X.external = k == 7              # the 7x7 conv is the encoder's first: external one-channel input
    Y = P.buf('Y', cout, oh, ow)
    P.input, P.output, P.x_c0, P.r_c0 = X, Y, 0, 0
    P.conv('T', X, 0, cin, Y, 0, cout, k, 2 if mode == 's2' else 1, k // 2, 1 if mode == 'up' else 0, 'T.weight')
    return P


@pytest.mark.parametrize('case', COUNT_CASES, ids=['k%d%s_%dx%d' % (c[0], c[1], c[4], c[5]) for c in COUNT_CASES])
def test_padding_counts_are_exact(case, device):
    k, mode, cin, cout, h, w = case
    B = sum(GROUPS)
    oh, ow = _out_plane(mode, h, w)
    prog = _count_program(*case)
    ones = lambda *s: torch.ones(*s, dtype=torch.float32)
    kw = dict(pool=ones(B, h * w)) if k == 7 else dict(x=ones(B, cin, h, w))
    r = _run(prog, GROUPS, device, {'T.weight': ones(cout, cin, k, k)}, 0.0, R=ones(B, cout, oh, ow), **kw)
    x = torch.ones(B, cin, h, w, dtype=torch.float64, requires_grad=True)
    wt = torch.ones(cout, cin, k, k, dtype=torch.float64, requires_grad=True)
    xi = F.interpolate(x, scale_factor=2, mode='nearest') if mode == 'up' else x
    y = F.conv2d(xi, wt, stride=2 if mode == 's2' else 1, padding=k // 2)
    y.sum().backward()
    assert tuple(y.shape) == (B, cout, oh, ow)
    assert (r['out T'].astype(np.float64) == y.detach().numpy()).all()
    assert k == 1 or float(y.detach().min()) < float(y.detach().max()), 'the case has no padding to count'
    o = r['offset']('T.weight')
    assert (r['gacc'][o:o + wt.numel()].reshape(wt.shape) == wt.grad.numpy()).all()
    if k != 7:
        assert (r['gin T'].astype(np.float64) == x.grad.numpy()).all()


# ---------------------------------------------------------------------------------------------- poison
# (k, mode, cin, cout, h, w, loss): T inside a producer / consumer chain, its planes at channel 1 of buffers of
# two more channels; 16 -> 8 on 32 x 32 stages the BN-backward operand as an LDS image, the others in registers
POISON_CASES = [(3, 's1', 6, 4, 16, 16, False), (3, 's1', 16, 8, 32, 32, False), (3, 's2', 5, 5, 16, 16, False),
                (3, 'up', 6, 6, 8, 8, False), (1, 's1', 5, 5, 8, 8, False), (7, 's2', 1, 6, 16, 16, False),
                (5, 's1', 3, 2, 16, 16, True)]


def _poison_program(k, mode, cin, cout, h, w, loss):
    P = CodecProgram('staging_poison')
    oh, ow = _out_plane(mode, h, w)
    stride, up = (2 if mode == 's2' else 1), (1 if mode == 'up' else 0)
    P.x_c0 = P.r_c0 = 0
    if k == 7:
        X = P.buf('input', 1, h, w)
        X.external = True
        P.input = X
        Y = P.buf('Y', cout + 2, oh, ow)
        P.conv('T', X, 0, 1, Y, 1, cout, 7, 2, 3, 0, 'T.weight')
    else:
        z = P.buf('z', 4, h, w)
        P.input = z
        X = P.buf('X', cin + 2, h, w)
        for i, c0 in enumerate(range(0, cin, L.GPI_MAX_COUT)):
            P.conv('p%d' % i, z, 0, 4, X, 1 + c0, min(L.GPI_MAX_COUT, cin - c0), 1, 1, 0, 0, 'p%d.weight' % i)
        if loss:
            Y = P.buf('out', 2, oh, ow)
            P.conv('T', X, 1, cin, Y, 0, cout, k, stride, k // 2, up, 'T.weight', bn='T.bn',
                   epilogue=L.EPI_GAUSS_LOSS)
            P.output = Y
            return P
        Y = P.buf('Y', cout + 2, oh, ow)
        P.conv('T', X, 1, cin, Y, 1, cout, k, stride, k // 2, up, 'T.weight', bn='T.bn')
    out = P.buf('out', 3, oh, ow)
    P.conv('c', Y, 1, cout, out, 0, 3, 1, 1, 0, 0, 'c.weight', bn='c.bn')
    P.output = out
    return P


def _poison_inputs(case, prog, B, pad):
    """Inputs of a poison case; `pad` fills what no kernel may read: unused pool and target rows."""
    k, mode, cin, cout, h, w, loss = case
    gen = torch.Generator().manual_seed(77 + k + cin)
    params = {}
    for op in prog.ops:
        params[op.w] = torch.randn(op.cout, op.cin, op.k, op.k, generator=gen) / float(np.sqrt(op.cin * op.k * op.k))
        if op.bn is not None:
            params[op.bn + '.weight'] = 0.5 + torch.rand(op.cin, generator=gen)
            params[op.bn + '.bias'] = torch.randn(op.cin, generator=gen) * 0.5
    kw = {}
    if k == 7:
        pool = torch.full((B + 2, h * w), pad)
        idx = torch.tensor([3, 1, 2][:B], dtype=torch.int32)        # rows 0 and 4 are nobody's
        pool[idx.long()] = torch.randn(B, h * w, generator=gen)
        kw.update(pool=pool, ext_idx=idx)
    else:
        kw['x'] = torch.randn(B, 4, h, w, generator=gen)
    o = prog.output
    if loss:
        tg, ti = [], []
        for n in GROUPS:
            t = torch.full((n + 2, o.H, o.W), pad)
            idx = torch.arange(1, n + 1, dtype=torch.int32).flip(0)   # rows 0 and n + 1 are nobody's
            t[idx.long()] = torch.randn(n, o.H, o.W, generator=gen)
            tg.append(t)
            ti.append(idx)
        kw.update(targets=tg, tgt_idx=ti)
    else:
        kw['R'] = torch.randn(B, o.C, o.H, o.W, generator=gen)
    return params, kw


@pytest.mark.parametrize('case', POISON_CASES,
                         ids=['k%d%s_%dto%d_%dx%d%s' % (c[:6] + ('_fused' if c[6] else '',)) for c in POISON_CASES])
def test_poisoned_neighbours_never_reach_a_result(case, device):
    B = sum(GROUPS)
    runs = {}
    for name, pad in (('clean', 0.0), ('poison', float('nan'))):
        for fused in ((False, True) if case[6] else (False,)):
            prog = _poison_program(*case)
            params, kw = _poison_inputs(case, prog, B, pad)
            runs[name, fused] = _run(prog, GROUPS, device, params, pad, fused=fused, **kw)
    for (name, fused), r in runs.items():
        if name != 'poison':
            continue
        ref = runs['clean', fused]
        for key, v in r.items():
            if key == 'offset':
                continue
            assert np.isfinite(v).all(), (key, fused)
            assert v.tobytes() == ref[key].tobytes(), (key, fused)
