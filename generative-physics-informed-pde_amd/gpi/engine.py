"""Execution engines: the ELBO training step and the standalone codec / ROM
operators, each a fixed sequence of libgpi_hip.so launches over
pre-planned workspaces.  No host synchronisation anywhere on the path.

ElboEngine = GenerativeModel.elbo (generative.py:247-287) for the armortized
unsupervised term (generative.py:546-585) + the supervised freeX term
(generative.py:461-500) + the virtual-observable freeX term
(generative.py:341-392, hold-off variant included), or their lockX variants
(independent_X = False: X~ = gp(z), generative.py:300-339,429-459), and its backward:

  forward   encoder program (B_u)            conv.hip  (11 launches at C64)
            dense head (all samples)          head.hip  (1)
            decoder program (B_u + N_s + N_vo, one BN group per term, fused Gaussian loss)  (12)
            ROM solve + log-lik + adjoint     rom.hip   (1 per labeled / VO term)
  backward  decoder program (reverse), dense head, encoder program (reverse),
            weight-gradient slab reduction, outer-product GEMMs, finalize.
"""
import ctypes as C
import os
import math
import warnings

import torch

from . import _lib as L
from .plan import Arena, encoder_program, decoder_program
from .schedule import MAIN, SIDE, E_ROM, E_DEC, E_ENC, E_SIDE, E_VALUE, step_schedule, walk

ENT_CONST = 0.5 * (math.log(2 * math.pi) + 1)
N_TERMS = 16
R = L.GPI_REPLICAS
# term slots in the fp64 scratch
T_LX0 = 0          # decoder Gaussian log-lik per group (0..3)
T_KL_ENC, T_KL_Q, T_LOGL_X, T_ENT = 4, 5, 6, 7           # head terms (supervised segment)
T_KL_Q2, T_LOGL_X2, T_ENT2 = 8, 9, 10                   # head terms (VO segment)
T_LOGL_Y, T_LOGL_Y2 = 11, 12                            # ROM log-lik (supervised, VO)


def groups_struct(sizes):
    g = L.Groups()
    g.n_groups = len(sizes)
    s = 0
    g.start[0] = 0
    for i, n in enumerate(sizes):
        s += n
        g.start[i + 1] = s
    for i in range(len(sizes) + 1, L.GPI_MAX_GROUPS + 1):
        g.start[i] = s
    return g


class Workspace(object):
    def __init__(self):
        self.ws = Arena()
        self.stats = Arena(align=1)
        self.parts = Arena()
        self.t_ws = None

    def alloc(self, n):
        return self.ws.alloc(n)

    def materialize(self, device):
        self.t_ws = torch.zeros(max(self.ws.size, 64), dtype=torch.float32, device=device)
        self.n_stats = max(self.stats.size, 1)
        self.t_scr = torch.zeros(N_TERMS * R + R * self.n_stats * L.GPI_MAX_GROUPS * 4 + 4, dtype=torch.float64,
                                 device=device)
        self.t_parts = torch.zeros(max(self.parts.size, 64), dtype=torch.float32, device=device)
        self.t_flag = torch.zeros(4, dtype=torch.int32, device=device)

    def view(self, off, *shape):
        n = 1
        for s in shape:
            n *= s
        return self.t_ws[off:off + n].view(*shape)

    def fptr(self, off):
        return C.c_void_p(self.t_ws.data_ptr() + 4 * off)

    @property
    def terms(self):
        """[N_TERMS] term sums (replica copies folded)."""
        return self.t_scr[:N_TERMS * R].view(N_TERMS, R).sum(1)

    def term_ptr(self, k):
        """Term slot k: GPI_REPLICAS consecutive fp64 accumulators."""
        return C.c_void_p(self.t_scr.data_ptr() + 8 * k * R)

    @property
    def stats_ptr(self):
        return C.c_void_p(self.t_scr.data_ptr() + 8 * N_TERMS * R)

    def zero_scratch(self):
        self.t_scr.zero_()


def gp_linears(gp):
    """The nn.Linear layers of an effective-property map (EffectivePropertyMap, or a bare deterministic map):
    the one Linear, or fc1 .. fc{L+1} of the MLP with L hidden layers (lamp/neuralnets.py)."""
    fc = gp.fc if hasattr(gp, 'fc') else gp
    return [fc] if isinstance(fc, torch.nn.Linear) else list(fc.linears)


def check_gp_hidden(n_hidden):
    if n_hidden > L.GPMLP_MAX_HIDDEN:
        raise L.NativeError('the effective-property map has %d hidden layers; the native path supports at most %d '
                            '(GPI_GPMLP_MAX_HIDDEN)' % (n_hidden, L.GPMLP_MAX_HIDDEN))


def make_ctx(ws, flat, group_sizes):
    c = L.CodecCtx()
    c.params = flat.P.data_ptr()
    c.ws = ws.t_ws.data_ptr()
    c.stats = ws.stats_ptr.value
    c.gacc = flat.gacc.data_ptr()
    c.wpart = ws.t_parts.data_ptr()
    c.ext_in = None
    c.ext_idx = None
    c.ext_stride = 0
    c.loss_acc = ws.term_ptr(T_LX0).value
    c.n_stats = ws.n_stats
    c.bn_eps = 1e-5
    c.groups = groups_struct(group_sizes)
    for g in range(L.GPI_MAX_GROUPS):
        c.loss_scale[g] = 1.0
    return c


HEAD_PARAMS = ('fc_w', 'fc_b', 'mu_w', 'mu_b', 'ls_w', 'ls_b', 'lat_w', 'lat_b', 'gp_w', 'gp_b', 'gp_ls', 'qz_mu',
               'qz_ls', 'qx_mu', 'qx_ls')
HEAD_PARAMS2 = ('qz_mu2', 'qz_ls2', 'qx_mu2', 'qx_ls2')
HEAD_BUFFERS = ('hpre', 'dhpre', 'zmu', 'zls', 'eps_z', 'z', 'gz', 'dzmu', 'dzls', 'eps_x', 'xs', 'mux', 'gxs', 'gmux')
ENC_HEAD = dict(fc_w='features.FC.weight', fc_b='features.FC.bias', mu_w='features.SplitDense.fc_mean.weight',
                mu_b='features.SplitDense.fc_mean.bias', ls_w='features.SplitDense.fc_logvar.weight',
                ls_b='features.SplitDense.fc_logvar.bias')
DEC_HEAD = dict(lat_w='latent_map.weight', lat_b='latent_map.bias')


def head_desc(hb, ws, second=False, **fields):
    """The HeadDesc builder of every engine: each parameter offset -1, each scale 1.0, the workspace buffers of hb,
    the term slots; a caller sets only what it uses (fields).  second: the second variational segment's offsets,
    scales and term slots too (ElboEngine); the codec engines have none (flags2 = 0: its fields are never read,
    and stay zero)."""
    h = L.HeadDesc()
    for k in HEAD_PARAMS + (HEAD_PARAMS2 if second else ()):
        setattr(h, k, -1)
    for k in ('kl_scale_enc', 'kl_scale_q', 'lx_scale') + (('kl_scale_q2', 'lx_scale2') if second else ()):
        setattr(h, k, 1.0)
    for k, v in hb.items():
        setattr(h, k, v)
    h.terms = ws.term_ptr(T_KL_ENC).value
    if second:
        h.terms2 = ws.term_ptr(T_KL_Q2).value
    for k, v in fields.items():
        setattr(h, k, v)
    return h


def codec_head_buffers(ws, B, dz, d_feat=0):
    """Head buffers of a standalone codec engine (the allocation order is the layout): the encoder's with
    hpre / dhpre [B, d_feat] first; the buffers it does not use at offset 0."""
    sizes = ([('hpre', d_feat), ('dhpre', d_feat)] if d_feat else []) + \
        [(k, dz) for k in ('zmu', 'zls', 'eps_z', 'z', 'gz', 'dzmu', 'dzls')]
    hb = {k: ws.alloc(B * n) for k, n in sizes}
    hb.update({k: 0 for k in HEAD_BUFFERS if k not in hb})
    return hb


def encoder_head(p, hb, ws, off, B, dz, train=True):
    """HeadDesc of a standalone encoder (program p): conv features -> (mean, logsigma)."""
    return head_desc(hb, ws, flags=L.HEAD_ENC, n_enc=B, n_q=0, d_feat=p.d_feat, d_z=dz, d_lat=1, d_x=1,
                     feat=p.output.off, gfeat=p.output.s_off if train else 0,
                     **{k: off(n) for k, n in ENC_HEAD.items()})


def decoder_head(p, hb, ws, off, B, dz, train=True):
    """HeadDesc of a standalone decoder (program p): the latent map z -> the first conv's input."""
    return head_desc(hb, ws, flags=L.HEAD_LATENT, n_enc=B, n_q=0, d_feat=1, d_z=dz, d_lat=p.input.per_sample, d_x=1,
                     lat=p.input.off, glat=p.input.s_off if train else 0, **{k: off(n) for k, n in DEC_HEAD.items()})


def gemm_item(a, b, S, M, N, lda, ldb, c, bias, flags=0):
    return L.GemmItem(a_off=a, b_off=b, c_off=c, bias_off=bias, S=S, M=M, N=N, lda=lda, ldb=ldb, flags=flags)


def encoder_head_gemms(h, hb, n):
    """Weight-gradient items of the encoder head's three Linear layers over its n samples."""
    dz, df = h.d_z, h.d_feat
    return [gemm_item(hb['dzmu'], hb['hpre'], n, dz, df, dz, df, h.mu_w, h.mu_b, 1),
            gemm_item(hb['dzls'], hb['hpre'], n, dz, df, dz, df, h.ls_w, h.ls_b, 1),
            gemm_item(hb['dhpre'], h.feat, n, df, df, df, df, h.fc_w, h.fc_b)]


def decoder_latent_gemms(h, hb, n):
    """Weight-gradient item of the decoder's latent map over its n samples."""
    return [gemm_item(h.glat, hb['z'], n, h.d_lat, h.d_z, h.d_lat, h.d_z, h.lat_w, h.lat_b)]


def gemm_array(items):
    return (L.GemmItem * len(items))(*items)


def codec_setup(e, kind, module, flat, B, train=True):
    """What the standalone codec engines (train and eval, 'enc' and 'dec') share, as attributes of e: the program
    p and its layout descs, the head buffers hb, the materialised workspace ws, the head descriptor and the codec
    context ctx.  Returns the module's parameter-offset function."""
    e.flat, e.B = flat, int(B)
    ws = e.ws = Workspace()
    off = lambda n: flat.offset(module.get_parameter(n))
    cfg = module.native_config()
    e.p = encoder_program(**cfg) if kind == 'enc' else decoder_program(final_epilogue=None, **cfg)
    e.descs = e.p.layout(e.B, ws.ws, ws.stats, ws.parts, groups_struct([e.B]), off, eval_mode=not train)
    e.dz = module.latent_dim if kind == 'enc' else module.dim_latent
    e.hb = codec_head_buffers(ws, e.B, e.dz, e.p.d_feat if kind == 'enc' else 0)
    ws.materialize(flat.P.device)
    e.head = (encoder_head if kind == 'enc' else decoder_head)(e.p, e.hb, ws, off, e.B, e.dz, train)
    e.ctx = make_ctx(ws, flat, [e.B])
    if kind == 'enc':
        e.ctx.ext_stride = e.p.input.per_sample
    return off


def _lib():
    return L.lib()


def head_forward(h, flat, ws, st, what='head forward'):
    _run(_lib().gpi_head_forward, C.byref(h), C.c_void_p(flat.P.data_ptr()), C.c_void_p(ws.t_ws.data_ptr()), st,
         what=what)


def head_backward(h, flat, ws, st, what='head backward'):
    _run(_lib().gpi_head_backward, C.byref(h), C.c_void_p(flat.P.data_ptr()), C.c_void_p(ws.t_ws.data_ptr()),
         C.c_void_p(flat.gacc.data_ptr()), st, what=what)


def outer_gemm(items, flat, ws, st):
    _run(_lib().gpi_outer_gemm, items, len(items), C.c_void_p(ws.t_ws.data_ptr()), C.c_void_p(flat.gacc.data_ptr()),
         st, what='outer gemm')


def run_reduce(items, ws, flat, st):
    """gpi_wgrad_reduce over a Python list of ReduceItem, in launches of <= GPI_MAX_REDUCE_ITEMS."""
    for k in range(0, len(items), L.GPI_MAX_REDUCE_ITEMS):
        part = items[k:k + L.GPI_MAX_REDUCE_ITEMS]
        arr = (L.ReduceItem * len(part))(*part)
        _run(_lib().gpi_wgrad_reduce, arr, len(part), C.c_void_p(ws.t_parts.data_ptr()),
             C.c_void_p(flat.gacc.data_ptr()), st, what='wgrad reduce')


def _run(fn, *args, what=None):
    L.check(fn(*args), what or fn.__name__)


def dropout_views(ws, progs):
    out = {}
    for key, prog, B in progs:
        if prog is None or prog.drop_numel == 0:
            continue
        out[key] = {name: ws.view(off, B, cout) for name, off, cout in prog.drop_ops()}
    return out


def draw_dropout(ws, progs, stream, seed, offset_ptr=None, sub=20, only=None):
    """Dropout2d scales of the programs (Philox sub id sub + position); only: the positions to draw."""
    for k, prog in enumerate(progs):
        if prog is None or prog.drop_numel == 0 or (only is not None and k not in only):
            continue
        _run(_lib().gpi_dropout_masks, ws.fptr(prog.drop_off), prog.drop_numel, prog.drop_rate, seed,
             offset_ptr, sub + k, stream, what='dropout masks')


class BnRunning(object):
    """BatchNorm2d running statistics of a set of codec programs (train mode, momentum 0.1):
    the reference updates running_mean / running_var / num_batches_tracked at every codec call;
    here one tiny launch per step folds every call's fp64 batch sums (gpi_bn_running_update)."""

    def __init__(self, entries, ws, device):
        """entries: [(program, module owning the BN layers, [(group, samples), ...] in call order)]."""
        items = []
        self.buffers = []
        max_ch = 1
        for prog, module, calls in entries:
            if prog is None or module is None or not calls:
                continue
            for op in prog.ops:
                if op.bn is None:
                    continue
                bn = module.get_submodule(op.bn)
                if bn.running_mean is None or bn.running_mean.device != device:
                    continue
                it = L.BnRunningItem()
                it.stat, it.channels, it.n_calls = op.desc.in_stat, op.cin, len(calls)
                for k, (g, n) in enumerate(calls):
                    it.group[k] = g
                    it.count[k] = float(n * op.src.H * op.src.W)
                it.running_mean, it.running_var = bn.running_mean.data_ptr(), bn.running_var.data_ptr()
                it.num_batches_tracked = bn.num_batches_tracked.data_ptr()
                items.append(it)
                self.buffers += [bn.running_mean, bn.running_var, bn.num_batches_tracked]
                max_ch = max(max_ch, op.cin)
        self.n = len(items)
        self.max_ch = max_ch
        self.ws = ws
        if self.n:
            arr = (L.BnRunningItem * self.n)(*items)
            raw = bytes(arr)
            self.dev = torch.tensor(list(raw), dtype=torch.uint8, device=device)

    def launch(self, stream, momentum=0.1):
        if self.n:
            _run(_lib().gpi_bn_running_update, C.c_void_p(self.dev.data_ptr()), self.n, self.max_ch,
                 self.ws.stats_ptr, self.ws.n_stats, momentum, stream, what='bn running stats')


def inject_dropout(views, masks):
    """Copy given channel scales {'enc' / 'dec': {conv name: [B, cout]}} into the engine's views."""
    for key, d in masks.items():
        for name, m in d.items():
            views[key][name].copy_(m)


class EventJoiner(object):
    """The schedule's edges as events: record on the signalling stream, wait_event on the waiting one
    (ElboEngine.handoff None).  streams: {MAIN / SIDE: (torch stream, launch handle)}."""

    def __init__(self, events, streams):
        self.ev, self.streams = events, streams

    def begin(self):
        pass

    def signal(self, edge, stream, fold):
        self.ev[edge].record(self.streams[stream][0])

    def wait(self, edge, stream):
        self.streams[stream][0].wait_event(self.ev[edge])

    def end(self):
        pass


class FlagJoiner(object):
    """Edges 0 .. 3 as device flags (gpi_stream_signal / gpi_stream_wait; ElboEngine.set_flag_handoff); a signal
    the table marks fold rides on the next main-stream piece's first conv launch.  E_VALUE stays an event."""

    def __init__(self, engine, events, main_wait):
        self.e, self.events, self.streams, self.main_wait = engine, events, events.streams, main_wait

    def begin(self):
        # the side stream's one fork of the step, before any of its kernels: its flag waits then
        # follow this step's signals only (never the previous step's); side_done: by the step counter
        e = self.e
        if e.side_done is not None:
            _, epoch, err = e.handoff
            _run(_lib().gpi_stream_wait_ge, C.c_void_p(epoch.data_ptr()), C.c_void_p(e.side_done.data_ptr()),
                 C.c_void_p(err.data_ptr()) if err is not None else None, self.streams[SIDE][1],
                 what='side step gate')
        else:
            self.events.signal('start', MAIN, False)
            self.events.wait('start', SIDE)

    def signal(self, edge, stream, fold):
        if edge == E_VALUE:
            return self.events.signal(edge, stream, fold)
        if fold:
            return edge
        self.e._signal(edge, self.streams[stream][1])

    def wait(self, edge, stream):
        if edge == E_VALUE:
            self.events.wait(edge, stream)
        elif edge != E_SIDE or self.main_wait:
            # (the side's end: a wait launch on the main chain, or folded into the caller's epilogue: main_wait False)
            self.e._wait(edge, self.streams[stream][1])

    def end(self):
        # side_done: the side stream's step ends by incrementing the counter its next step gate reads; else the
        # event join (capture legality) after the step's last kernel: rejoin()
        e = self.e
        if e.side_done is not None:
            _run(_lib().gpi_rng_advance, C.c_void_p(e.side_done.data_ptr()), 1, self.streams[SIDE][1],
                 what='side step done')
        else:
            self.events.signal(E_SIDE, SIDE, False)
            e._rejoin_pending = True


class ElboEngine(object):
    """Fused armortized-unsupervised + supervised-freeX (+ virtual-observable freeX) ELBO of a
    GenerativeModel.  N_vo > 0 adds the VO term (its own decoder BN group, q_z['vo'] / q_X['vo']
    rows as the head's second variational segment, a second ROM launch against targets sampled
    from the VO posterior); vo_holdoff keeps only its logL_x - KL part (generative.py:349-364)."""

    def __init__(self, model, B_u, N_s, normalize=False, N_vo=0, vo_holdoff=False, q_unsup=None,
                 running_modules=None, shared_grads=True, y_weight=None):
        """q_unsup: q_z['unsupervised'] for the non-armortized unsupervised term (no encoder,
        GenerativeModel.elbo_unsupervised generative.py:515-544): its rows replace the encoder
        heads; the term's KL is the reference's KLD of q_z['supervised'] (sic, :525).
        shared_grads=False: gradients of the per-sample variational rows only -- the codec backward
        computes input gradients without weight / BN-affine gradients (no slab rows, no slab
        reductions) and the dense weight GEMM is skipped (the PredictionEnsemble, whose Adam updates
        its q_z rows only while the reference discards the decoder gradients it also forms)."""
        self.shared_grads = bool(shared_grads)
        self.model = model
        self.q_unsup = q_unsup
        self.armortized = q_unsup is None
        self.flat = model._flat
        self.B_u, self.N_s, self.N_vo = int(B_u), int(N_s), int(N_vo)
        self.vo_holdoff = bool(vo_holdoff) and self.N_vo > 0
        self.N_q = self.N_s + self.N_vo
        self.B = self.B_u + self.N_q
        self.normalize = bool(normalize)
        # q samples whose X~ enters the ROM / gp likelihood (hold-off VO samples do not)
        self.N_x = self.N_s + (self.N_vo if not self.vo_holdoff else 0)
        enc, dec, gp, g = model.encoder, model.f, model.gp, model.g
        # lockX (independent_X = False): X~ = gp(z), no q_X rows, no q_X noise, no logL_X / entropy
        self.lockx = not gp.independent_X
        self.N_ex = 0 if self.lockx else self.N_x
        self.enc, self.dec, self.gp, self.g = enc, dec, gp, g
        self.dz = dec.dim_latent
        self.ws = Workspace()
        self._build_layout()
        self._build_head()
        self._build_gemm_items()
        self._build_roms(y_weight)
        self._build_switches(running_modules or {})

    def _poff(self, mod, name):
        return self.flat.offset(mod.get_parameter(name))

    def _build_layout(self):
        """Programs and workspace layout: ep / enc_descs, dp / dec_descs, n_enc_conv, n_dec_sep, the head
        buffers hb, gp_mlp_buffers, gls_off, the materialised workspace and the codec contexts ectx / dctx.  The
        order of the allocations is the layout: every workspace offset, and so every descriptor, follows it."""
        model, flat, ws, dz = self.model, self.flat, self.ws, self.dz
        enc, dec, gp, g = self.enc, self.dec, self.gp, self.g
        # ---- encoder program
        if self.B_u > 0 and self.armortized:
            self.ep = encoder_program(**enc.native_config())
            self.enc_descs = self.ep.layout(self.B_u, ws.ws, ws.stats, ws.parts, groups_struct([self.B_u]),
                                            lambda n: self._poff(enc, n))
            d_feat = self.ep.d_feat
        else:
            self.ep = None
            d_feat = 1
        self.d_feat = d_feat
        # ---- decoder program (groups: unsup, sup, vo)
        dc = dec.native_config()
        # the decoder likelihood of generative.py:232-244: log-property Gaussian (default) or the
        # exponentiated field's (reconstruct_log_eff_property = False); a binary decoder (one logit channel)
        # takes the Bernoulli likelihood whatever that option says -- the reference tests the prediction's
        # type first.  A homoscedastic decoder (one mean channel + the learned log-sigma plane f.logsigma,
        # Decoder.py:204-212,271-285) takes the same Gaussian of either field with log sigma read from the plane
        log_field = getattr(model, 'config', {}).get('reconstruct_log_eff_property', True)
        self.binary = bool(getattr(dec, '_binary', False))
        self.homosc = bool(getattr(dec, '_homoscedastic', False)) and not self.binary
        if self.binary:
            epi = L.EPI_BERNOULLI_LOSS
        elif self.homosc:
            epi = L.EPI_GAUSS_HOMO_LOSS if log_field else L.EPI_GAUSS_HOMO_EXP_LOSS
        else:
            epi = L.EPI_GAUSS_LOSS if log_field else L.EPI_GAUSS_EXP_LOSS
        self.dp = decoder_program(final_epilogue=epi, **dc)
        self.dec_sizes = [n for n in (self.B_u, self.N_s, self.N_vo) if n > 0]
        self.g_sup = (1 if self.B_u > 0 else 0) if self.N_s > 0 else None
        self.g_vo = ((self.B_u > 0) + (self.N_s > 0)) if self.N_vo > 0 else None
        self.dec_descs = self.dp.layout(self.B, ws.ws, ws.stats, ws.parts, groups_struct(self.dec_sizes),
                                        lambda n: self._poff(dec, n))
        # codec launch ranges: the encoder's ops [0, n_enc_conv), the decoder's [0, n_dec_sep) (+ the fused output
        # conv); dec0 = 0 is read by bench.py's launch list only
        self.n_enc_conv = len(self.enc_descs) if self.ep is not None else 0
        self.dec0 = 0
        # the loss epilogue consumes (mu, logsigma) in registers: nobody reads the output image (9.4 MB of
        # writes per step at C64)
        self.dec_descs[len(self.dec_descs) - 1].out_off = -1
        if not self.shared_grads:
            for d in self.dec_descs:
                d.wpart_off = -1          # input gradients only
        # the output conv's forward and backward run as ONE launch at the end of the forward
        # (gpi_conv_loss_fused: the loss gradient stays in LDS); GPI_FUSE_OUT=0 keeps them apart (A/B only)
        self.n_dec_sep = len(self.dec_descs) - (1 if os.environ.get('GPI_FUSE_OUT', '1') != '0' else 0)
        # ---- dense head buffers
        self.d_lat = self.dp.input.per_sample
        d_x = g.dim_effective_property if self.N_q > 0 else 1
        self.d_x = d_x
        self.d_y = g.dim_out
        # nonlinear effective-property map (L hidden layers): gpi_gpmlp_forward / _backward own the gp term of the
        # q rows, the head runs without GPI_HEAD_GP.  L = 0: nothing of this exists -- no launch, no buffer.
        self.gp_lin = gp_lin = gp_linears(gp) if self.N_x > 0 else []
        self.gp_hidden = max(len(gp_lin) - 1, 0)
        check_gp_hidden(self.gp_hidden)
        self.gp_widths = ([gp_lin[0].in_features] + [fc.out_features for fc in gp_lin]) if self.gp_hidden else []
        hb = {}
        for name, n in (('hpre', self.B_u * d_feat), ('dhpre', self.B_u * d_feat),
                        ('zmu', self.B * dz), ('zls', self.B * dz), ('eps_z', self.B * dz), ('z', self.B * dz),
                        ('gz', self.B * dz), ('dzmu', self.B * dz), ('dzls', self.B * dz),
                        ('eps_x', self.N_q * d_x), ('xs', self.N_q * d_x), ('mux', self.N_q * d_x),
                        ('gxs', self.N_q * d_x), ('gmux', self.N_q * d_x),
                        ('y_vo', (self.N_vo if not self.vo_holdoff else 0) * self.d_y)):
            hb[name] = ws.alloc(max(n, 1))
        self.hb = hb
        # h_k / delta_k [N_x, width_k] of the MLP's hidden layers
        self.gp_mlp_buffers = {}
        for k in range(1, self.gp_hidden + 1):
            for name in ('h%d' % k, 'dh%d' % k):
                self.gp_mlp_buffers[name] = ws.alloc(self.N_x * self.gp_widths[k])
        self.gp_mlp_launches = 2 if self.gp_hidden else 0
        # ROM log-likelihood: per-sample d/dlogsigma_y rows (plain stores), reduced into gacc with the
        # decoder slabs (gpi_rom gls_part) -- instead of n x d_y same-address fp64 atomics
        self.gls_off = {}
        for key, n in (('sup', self.N_s), ('vo', 0 if self.vo_holdoff else self.N_vo)):
            if n > 0:
                self.gls_off[key] = ws.parts.alloc(n * self.d_y)
        # homoscedastic decoder: the per-sample d/dlogsigma rows [B][H W] of the plane, written by the loss
        # epilogue and summed over the batch with the decoder slabs; none without shared_grads (the plane is read,
        # its gradient never formed)
        self.dec_gls_off = -1
        if self.homosc and self.shared_grads:
            self.dec_gls_off = ws.parts.alloc(self.B * self.dp.output.per_sample)
        ws.materialize(flat.P.device)
        su = 1.0 / self.B_u if (self.normalize and self.B_u) else 1.0
        ss = 1.0 / self.N_s if (self.normalize and self.N_s) else 1.0
        sv = 1.0 / self.N_vo if (self.normalize and self.N_vo) else 1.0
        self.su, self.ss, self.sv = su, ss, sv
        # ---- contexts
        if self.ep is not None:
            self.ectx = make_ctx(ws, flat, [self.B_u])
            self.ectx.ext_stride = self.ep.input.per_sample
        self.dctx = make_ctx(ws, flat, self.dec_sizes)
        for gi, scale in enumerate([su] * (self.B_u > 0) + [ss] * (self.N_s > 0) + [sv] * (self.N_vo > 0)):
            self.dctx.loss_scale[gi] = scale
        if self.homosc:
            self.dctx.ls_off = flat.offset(dec.logsigma)
            self.dctx.gls_off = self.dec_gls_off

    def _build_head(self):
        """The dense head's descriptor (head) and the MLP effective-property map's (gpm, or None)."""
        model, flat, ws, hb, gp, dz = self.model, self.flat, self.ws, self.hb, self.gp, self.dz
        su, ss, sv = self.su, self.ss, self.sv
        gp_lin = self.gp_lin
        gpf = (L.HEAD_GP | (L.HEAD_LOCKX if self.lockx else 0)) if not self.gp_hidden else 0
        flags = L.HEAD_LATENT
        if self.B_u > 0:
            flags |= (L.HEAD_ENC if self.armortized else 0) | L.HEAD_REPARAM
        if self.N_s > 0:
            flags |= L.HEAD_QZ | gpf
        f = dict(flags=flags, n_enc=self.B_u, n_q=self.N_s, n_q2=self.N_vo, d_feat=self.d_feat, d_z=dz,
                 d_lat=self.d_lat, d_x=self.d_x, lat=self.dp.input.off, glat=self.dp.input.s_off,
                 kl_scale_enc=su, kl_scale_q=ss, lx_scale=ss, kl_scale_q2=sv, lx_scale2=sv)
        f.update({k: self._poff(self.dec, n) for k, n in DEC_HEAD.items()})
        if self.N_vo > 0:
            f['flags2'] = L.HEAD_QZ | (0 if self.vo_holdoff else gpf)
        if self.ep is not None:
            f.update({k: self._poff(self.enc, n) for k, n in ENC_HEAD.items()})
            f.update(feat=self.ep.output.off, gfeat=self.ep.output.s_off)
        if self.N_x > 0 and not self.gp_hidden:
            f.update(gp_w=self._poff(gp, 'fc.weight'), gp_b=self._poff(gp, 'fc.bias'))
            if not self.lockx:
                f['gp_ls'] = self._poff(gp, 'logsigmas_X')
        # q rows: (segment suffix, key, has free-X rows)
        for sfx, key, n, qx in (('', 'supervised', self.N_s, not self.lockx),
                                ('2', 'vo', self.N_vo, not self.vo_holdoff and not self.lockx)):
            if n > 0:
                q = model.q_z[key]
                f['qz_mu' + sfx], f['qz_ls' + sfx] = flat.offset(q._mean), flat.offset(q._logsigma)
                if qx:
                    q = model.q_X[key]
                    f['qx_mu' + sfx], f['qx_ls' + sfx] = flat.offset(q._mean), flat.offset(q._logsigma)
        if not self.armortized and self.B_u > 0:
            if self.N_s == 0:
                raise KeyError("elbo_unsupervised takes the KL of q_z['supervised'] (generative.py:525)")
            # the unsupervised term's KL is q_z['supervised']'s: no KL gradient on q_z['unsupervised'],
            # a second one (scale su) on the supervised rows
            f.update(kl_scale_enc=0.0, kl_scale_q=ss + su)
        self.head = h = head_desc(hb, ws, second=True, **f)
        self.gpm = None
        if self.gp_hidden:
            m = L.GpMlpDesc()
            m.n_layers, m.n1, m.n2 = self.gp_hidden, self.N_s, self.N_x - self.N_s
            m.flags = L.GPMLP_LOCKX if self.lockx else 0
            for k, w in enumerate(self.gp_widths):
                m.width[k] = w
            for k in range(L.GPMLP_MAX_HIDDEN + 1):
                m.w[k] = flat.offset(gp_lin[k].weight) if k < len(gp_lin) else -1
                m.b[k] = flat.offset(gp_lin[k].bias) if k < len(gp_lin) else -1
            m.gp_ls = self._poff(gp, 'logsigmas_X') if not self.lockx else -1
            for k in ('qx_mu', 'qx_ls', 'qx_mu2', 'qx_ls2', 'qz_mu', 'qz_ls', 'qz_mu2', 'qz_ls2'):
                setattr(m, k, getattr(h, k))
            m.z, m.eps_z = hb['z'] + self.B_u * dz, hb['eps_z'] + self.B_u * dz
            for k in range(L.GPMLP_MAX_HIDDEN):
                m.h[k] = self.gp_mlp_buffers.get('h%d' % (k + 1), -1)
                m.dh[k] = self.gp_mlp_buffers.get('dh%d' % (k + 1), -1)
            for k in ('eps_x', 'xs', 'mux', 'gxs', 'gmux'):
                setattr(m, k, hb[k])
            m.dz = -1
            m.lx_scale, m.lx_scale2 = ss, sv
            m.terms = ws.term_ptr(T_LOGL_X).value
            m.terms2 = ws.term_ptr(T_LOGL_X2).value
            self.gpm = m

    def _build_gemm_items(self):
        """gemm_items: the dense layers' weight-gradient outer products (none without shared_grads)."""
        h, hb, dz, d_x = self.head, self.hb, self.dz, self.d_x
        z_q = hb['z'] + self.B_u * dz           # the q samples' rows of z
        gi = decoder_latent_gemms(h, hb, self.B)
        if self.N_x > 0 and not self.gp_hidden:
            gi.append(gemm_item(hb['gmux'], z_q, self.N_x, d_x, dz, d_x, dz, h.gp_w, h.gp_b))
        for k in range(1, self.gp_hidden + 2) if self.gp_hidden else ():
            # layer k of the MLP: sum over rows of delta_k (x) h_{k-1} (delta_{L+1} = gmux, h_0 = z)
            wo, wi = self.gp_widths[k], self.gp_widths[k - 1]
            a = hb['gmux'] if k == self.gp_hidden + 1 else self.gp_mlp_buffers['dh%d' % k]
            b = z_q if k == 1 else self.gp_mlp_buffers['h%d' % (k - 1)]
            gi.append(gemm_item(a, b, self.N_x, wo, wi, wo, wi, self.gpm.w[k - 1], self.gpm.b[k - 1]))
        if self.ep is not None:
            gi += encoder_head_gemms(h, hb, self.B_u)
        self.gemm_items = gemm_array(gi if self.shared_grads else [])

    def _build_roms(self, y_weight):
        """The ROM descriptors (one launch per labeled / VO term; both on the side stream) and the slab
        reductions: rom_draw, y_weight, roms / rom / rom_vo, reduce_enc, n_reduce_in, reduce_dec, reduce_items."""
        model, flat, ws, hb, g, d_x = self.model, self.flat, self.ws, self.hb, self.g, self.d_x
        ss, sv = self.ss, self.sv
        offE = lambda n: self._poff(self.enc, n)
        self.reduce_enc = self.ep.reduce_items(offE) if self.ep is not None else []
        # slab-reduction items of the encoder's input conv (the first op; no input BN: one item)
        # (counted per op: 1 for the weight, +1 or +2 for an input BN whose gamma / beta are (not)
        # adjacent; a miscount would leave one of its items to the side stream while the main
        # stream's input-conv backward still writes that slab)
        self.n_reduce_in = self.ep.reduce_counts(offE)[0] if self.ep is not None else 0

        def rom_desc(row0, n, scale, slot):
            r = L.RomDesc()
            rom = g.rom
            r.nc, r.refine, r.n, r.mode = rom.nc, rom.refine, n, L.ROM_LOGLIK
            r.x = ws.fptr(hb['xs'] + row0 * d_x).value
            r.x_stride = d_x
            r.logsig_y = flat.P.data_ptr() + 4 * flat.offset(g.logsigmas_y)
            r.loss_scale = scale
            r.gx_accumulate = 0
            if self.rom_draw:
                # the ROM draws its X~ rows from q_X itself (no wait on the head forward's xs)
                qx = model.q_X['supervised' if slot == T_LOGL_Y else 'vo']
                r.x_draw = 1
                r.x_mu = flat.P.data_ptr() + 4 * flat.offset(qx._mean)
                r.x_ls = flat.P.data_ptr() + 4 * flat.offset(qx._logsigma)
                r.x_eps = ws.fptr(hb['eps_x'] + row0 * d_x).value
            r.gx = ws.fptr(hb['gxs'] + row0 * d_x).value
            r.gx_stride = d_x
            r.gacc_logsig = flat.gacc.data_ptr() + 8 * flat.offset(g.logsigmas_y)
            r.loss_acc = ws.term_ptr(slot).value
            r.flag = ws.t_flag.data_ptr()
            r.mu_y = None
            r.uc = None
            r.dmu = None
            if slot == T_LOGL_Y and self.y_weight is not None:
                # partially observed labels: the supervised launch alone (virtual observables are complete);
                # the unobserved entries' d/dlogsigma_y rows are zeros, so the reduce item below is unchanged
                r.y_weight = self.y_weight.data_ptr()
                r.yw_stride = self.d_y if self.y_weight.dim() == 2 else 0
            key = 'sup' if slot == T_LOGL_Y else 'vo'
            r.gls_part = ws.t_parts.data_ptr() + 4 * self.gls_off[key]
            it = L.ReduceItem()
            it.part_off, it.w_off, it.numel, it.row_stride, it.blocks = (self.gls_off[key], flat.offset(g.logsigmas_y),
                                                                         self.d_y, self.d_y, n)
            self.rom_reduce.append(it)
            return r

        self.rom_reduce = []
        # observation weights of the labelled term (GenerativeModel.label_weights): fp32 [d_y] shared or
        # [N_s, d_y]; the descriptor holds the tensor's address, the engine keeps the tensor
        if y_weight is not None:
            L.require_device(y_weight)
            if y_weight.dtype != torch.float32 or not y_weight.is_contiguous() or \
                    tuple(y_weight.shape) not in ((self.d_y,), (self.N_s, self.d_y)):
                raise ValueError('y_weight: contiguous fp32 [%d] or [%d, %d], got %s %s'
                                 % (self.d_y, self.N_s, self.d_y, y_weight.dtype, tuple(y_weight.shape)))
        self.y_weight = y_weight if self.N_s > 0 else None
        # GPI_ROM_EARLY=1 (free q_X only): the fused step's ROM runs at the very start of the step on
        # the side stream, its inputs drawn from q_X in the kernel, concurrently with the encoder
        # (not with the MLP map, whose forward runs ahead of the ROM on the side stream and needs the head's z)
        self.rom_draw = os.environ.get('GPI_ROM_EARLY', '0') == '1' and not self.lockx and not self.gp_hidden
        if os.environ.get('GPI_ROM_EARLY', '0') == '1' and self.gp_hidden and self.N_x > 0:
            warnings.warn('GPI_ROM_EARLY=1 is ignored: the effective-property map has hidden layers, whose forward '
                          'runs ahead of the ROM and needs the head forward (the default ROM order is used)')
        self.roms = []
        self.rom = self.rom_vo = None
        if self.N_s > 0:
            self.rom = rom_desc(0, self.N_s, ss, T_LOGL_Y)
            self.roms.append(self.rom)
        if self.N_vo > 0 and not self.vo_holdoff:
            self.rom_vo = rom_desc(self.N_s, self.N_vo, sv, T_LOGL_Y2)
            self.rom_vo.Y = ws.fptr(hb['y_vo']).value
            self.roms.append(self.rom_vo)
        # the ROMs' d/dlogsigma_y rows are reduced with the decoder slabs (after the ROMs on the side stream)
        dec_items = self.dp.reduce_items(lambda n: self._poff(self.dec, n)) if self.shared_grads else []
        if self.dec_gls_off >= 0:
            # the homoscedastic plane's gradient: the cross-batch sum of the epilogue's per-sample rows
            it = L.ReduceItem()
            hw = self.dp.output.per_sample
            it.part_off, it.w_off, it.numel, it.row_stride, it.blocks = (self.dec_gls_off, flat.offset(self.dec.logsigma),
                                                                         hw, hw, self.B)
            dec_items.append(it)
        self.reduce_dec = dec_items + self.rom_reduce
        self.reduce_items = self.reduce_enc + self.reduce_dec

    def _build_switches(self, run_mods):
        """BN running statistics, the scheduling switches (enc_reduce, rom_first, rom_at, side_pre), SyncBN and
        hand-off state."""
        self._side = None
        # BN running statistics: encoder once, decoder once per term in the reference's call order
        # (unsupervised, supervised, vo: generative.py:247-287)
        self.running = BnRunning([(self.ep, run_mods.get('enc', self.enc), [(0, self.B_u)]),
                                  (self.dp, run_mods.get('dec', self.dec), list(enumerate(self.dec_sizes)))],
                                 self.ws, self.flat.P.device)
        # encoder slab reduction: all on the main stream after the input conv's backward ('main'), or
        # split ('split': the input conv's slabs on the main stream, the rest on the side stream
        # concurrently with the input conv's backward)
        self.enc_reduce = os.environ.get('GPI_ENC_REDUCE', 'split')
        # ROM launches enqueued before the decoder forward (capture order) instead of after it
        self.rom_first = False
        # where the fused step's ROM forks to the side stream: after the head forward ('forward') or
        # with the backward's side work ('backward'; GPI_ROM_AT)
        # (A/Bs within the boxes' +-1 % noise: 'backward' 0.6308 / 0.6286 vs 0.6370 / 0.6332 ms on one box,
        # 0.6277 / 0.6274 / 0.6316 / 0.6342 / 0.6485 vs 'forward' 0.6240 / 0.6255 / 0.6303 / 0.6255 / 0.6336 on
        # two others, r03: kept 'forward')
        self.rom_at = os.environ.get('GPI_ROM_AT', 'forward')
        self.rom_early_launched = False
        # the schedule of the step in flight (forward() -> backward()); its ROM still to run with the backward
        self._sched = None
        self._rom_deferred = False
        # callable(side stream handle) launched on the side stream ahead of the ROM (fused step)
        self.side_pre = None
        # SyncBN (set_sync_bn): None = replica-BN, per-rank batch statistics
        self.bn_sync = None
        self.bn_world = 1
        # cross-stream hand-offs: graph events (None) or device flags (set_flag_handoff)
        self.handoff = None
        self.side_done = None
        self._rejoin_pending = False

    # ------------------------------------------------------------------
    def set_flag_handoff(self, flags, epoch, err=None, side_done=None):
        """Hand the side stream its work by device flags (gpi_stream_signal / gpi_stream_wait) instead of
        event edges between the streams: flags = int32 device tensor (>= 4 words), epoch = the step
        counter (int64 device tensor, constant within a step), err = an int32 word the waits set on a
        timeout.  The side stream forks from the main stream once at the start of the forward; after
        the step's last kernel the caller joins it back with rejoin() (stream-capture legality: the
        events there sit at the graph's end, not between kernels of the main chain).
        side_done (int64 device counter): the streams are not joined by events at all -- the side
        stream's step starts with a wait until the step counter has reached side_done (the main stream's
        previous step has ended) and ends by incrementing it, so each stream can be captured as a
        graph of its own (FusedElboStep graph_mode 'streams')."""
        self.handoff = (flags, epoch, err)
        self.side_done = side_done

    def _signal(self, k, st):
        f, e, _ = self.handoff
        _run(_lib().gpi_stream_signal, C.c_void_p(f.data_ptr() + 4 * k), C.c_void_p(e.data_ptr()), st,
             what='stream signal')

    def _sig_args(self, k):
        """(flag, epoch) pointers of hand-off flag k for the *_sig launches (signal folded into a conv)."""
        f, e, _ = self.handoff
        return C.c_void_p(f.data_ptr() + 4 * k), C.c_void_p(e.data_ptr())

    def _wait(self, k, st):
        f, e, err = self.handoff
        _run(_lib().gpi_stream_wait, C.c_void_p(f.data_ptr() + 4 * k), C.c_void_p(e.data_ptr()),
             C.c_void_p(err.data_ptr()) if err is not None else None, st, what='stream wait')

    def rejoin(self):
        """Main stream waits for the side stream's end (flag hand-off mode; a no-op otherwise)."""
        if self._rejoin_pending:
            torch.cuda.current_stream().wait_event(self._ev[E_SIDE])
            self._rejoin_pending = False

    def _head_part(self, part, st):
        """Head backward of one half of the samples (HEAD_PART_ENC / HEAD_PART_Q: the split rule)."""
        hd = L.HeadDesc.from_buffer_copy(self.head)
        hd.flags |= part
        head_backward(hd, self.flat, self.ws, st)

    def _gp_forward(self, st):
        _run(_lib().gpi_gpmlp_forward, C.byref(self.gpm), C.c_void_p(self.flat.P.data_ptr()),
             C.c_void_p(self.ws.t_ws.data_ptr()), st, what='gp mlp forward')

    def _gp_backward(self, st):
        _run(_lib().gpi_gpmlp_backward, C.byref(self.gpm), C.c_void_p(self.flat.P.data_ptr()),
             C.c_void_p(self.ws.t_ws.data_ptr()), C.c_void_p(self.flat.gacc.data_ptr()), st, what='gp mlp backward')

    def eps_z(self):
        return self.ws.view(self.hb['eps_z'], self.B, self.dz)

    @property
    def has_dropout(self):
        return any(p is not None and p.drop_numel > 0 for p in (self.ep, self.dp))

    def dropout_views(self):
        """{'enc': {conv name: [B_u, cout]}, 'dec': {conv name: [B, cout]}}: the Dropout2d channel
        scales (0 or 1/(1-p)) the next forward uses."""
        return dropout_views(self.ws, (('enc', self.ep, self.B_u), ('dec', self.dp, self.B)))

    def draw_dropout(self, stream, seed, offset_ptr=None, sub=20, codecs=('enc', 'dec')):
        """Fresh Dropout2d scales for every dropout conv of the codecs (device Philox; the encoder's
        stream is sub, the decoder's sub + 1 whichever are drawn)."""
        draw_dropout(self.ws, (self.ep, self.dp), stream, seed, offset_ptr, sub,
                     only=[k for k, c in enumerate(('enc', 'dec')) if c in codecs])

    def eps_x(self):
        """[N_ex, d_x] q_X noise (supervised rows, then VO rows unless held off; none in lockX)."""
        return self.ws.view(self.hb['eps_x'], self.N_ex, self.d_x)

    def y_vo(self):
        """[N_vo, d_y] VO targets y ~ N(VO.mean, VO.var) of this step (generative.py:356)."""
        return self.ws.view(self.hb['y_vo'], self.N_vo if not self.vo_holdoff else 0, self.d_y)

    def bind(self, X_u=None, u_index=None, X_s=None, Y=None, F=None, X_vo=None, F_vo=None):
        """Point the launch descriptors at this step's data tensors.  The engine keeps them alive
        until the next bind: the backward reads X_u again (the input conv's weight gradient), so a
        caller's temporary (e.g. a random-subset gather) must not return to the allocator between
        the forward and the backward.
        Binary decoder: each bound group's low-phase value tgt_lo = the minimum of the tensor bound to it
        (the reference's target == target.min() rule, generative.py:241-242; for X_u with u_index that is
        the pool's minimum) -- one torch reduction and host read (a device synchronisation) per bound tensor,
        outside any captured step, and only when the tensor is new: the minimum is kept per (storage, version,
        shape), so the module path's repeated elbo() calls on the same dataset tensors do not synchronise again."""
        self._bound = (X_u, u_index, X_s, Y, F, X_vo, F_vo)
        if self.binary:
            for gi, t in ((0 if self.B_u > 0 else None, X_u), (self.g_sup, X_s), (self.g_vo, X_vo)):
                if gi is not None:
                    self.dctx.tgt_lo[gi] = self._target_low(t)
        if self.B_u > 0:
            L.require_device(X_u)
            assert X_u.dtype == torch.float32 and X_u.is_contiguous()
            if self.armortized:
                self.ectx.ext_in = X_u.data_ptr()
                self.ectx.ext_idx = u_index.data_ptr() if u_index is not None else None
            else:
                assert X_u.shape[0] == self.B_u and u_index is None
            self.dctx.tgt[0] = X_u.data_ptr()
            self.dctx.tgt_idx[0] = u_index.data_ptr() if u_index is not None else None
        if self.N_s > 0:
            gs = 1 if self.B_u > 0 else 0
            for t in (X_s, Y, F):
                L.require_device(t)
                assert t.dtype == torch.float32 and t.is_contiguous()
            self.dctx.tgt[gs] = X_s.data_ptr()
            self.dctx.tgt_idx[gs] = None
            self.rom.Y = Y.data_ptr()
            self.rom.F = F.data_ptr()
        if self.N_vo > 0:
            for t in (X_vo,) + ((F_vo,) if not self.vo_holdoff else ()):
                L.require_device(t)
                assert t.dtype == torch.float32 and t.is_contiguous()
            assert X_vo.shape[0] == self.N_vo
            self.dctx.tgt[self.g_vo] = X_vo.data_ptr()
            self.dctx.tgt_idx[self.g_vo] = None
            if not self.vo_holdoff:
                assert F_vo.shape[0] == self.N_vo
                self.rom_vo.F = F_vo.data_ptr()

    def _target_low(self, t):
        """min(t) of a bound target tensor, read to the host once per (storage, in-place version, shape).  An
        entry keeps its tensor alive, so the allocator cannot hand its address to other data while the entry
        stands; a random-subset gather is a new tensor every call and takes the reduction every time."""
        key = (t.data_ptr(), t._version, tuple(t.shape))
        cache = self.__dict__.setdefault('_tgt_lo_cache', {})
        if key not in cache:
            if len(cache) >= 8:
                cache.clear()
            cache[key] = (t, float(t.min().item()))
        return cache[key][1]

    def forward(self, stream=None, compute_value=True, zero_gacc=True, zero_scratch=True, running='now'):
        """Launch the forward; returns the 0-d ELBO tensor (no host sync).  zero_gacc / zero_scratch
        False when the previous step's epilogue already cleared the accumulator / the statistics
        and term scratch (gpi_step_epilogue).  running: BN running-statistics update 'now' (end of
        the forward), 'defer' (on the side stream during backward) or None."""
        st = stream if stream is not None else L.stream_handle()
        # early ROM: after the side gate (the previous step's update and epilogue -- q_X, eps_x, the
        # cleared term scratch -- are complete); needs the gate and a scratch this forward does not clear
        early = self.rom_draw and self.side_done is not None and not zero_scratch
        self._sched = self.schedule(compute_value, running, early)
        self.rom_early_launched = self._sched.forward[0].stream == SIDE
        self._rom_deferred = any(s.args.get('rom') for s in self._sched.backward)
        joiner = self._joiner(st)
        joiner.begin()
        self._walk(self._sched.forward, joiner, forward_a=dict(zero_gacc=zero_gacc, zero_scratch=zero_scratch))
        return self.elbo_value() if compute_value else None

    def backward(self, stream=None, side_extra=None, main_wait=True):
        """Gradients of -ELBO into flat.gacc (fp64).  side_extra(side_stream_handle) is launched on
        the side stream after the decoder's reductions, concurrently with the encoder backward (the
        fused step draws the next step's subset, noise and decoder dropout masks there; nothing it
        writes may be read by the encoder backward).  main_wait=False (flag hand-off only): the main
        stream does not wait for the side stream's end here -- the caller's next launch does
        (gpi_step_epilogue_adam wait_flag)."""
        st = stream if stream is not None else L.stream_handle()
        joiner = self._joiner(st, main_wait)
        self._walk(self._sched.backward, joiner, backward_side_a=dict(side_extra=side_extra))
        self._rom_deferred = False
        joiner.end()

    def schedule(self, compute_value, running, early=False, segments=False):
        """The step's schedule table (gpi.schedule) for the engine's switches as they stand now.  segments: the
        table FusedElboStep's segment graphs are captured from, which has no rom_at / rom_first arm."""
        return step_schedule(self.n_enc_conv, bool(self.roms), self.enc_reduce,
                             'forward' if segments else self.rom_at, not segments and self.rom_first, early,
                             compute_value, running)

    def _joiner(self, st, main_wait=True):
        side = self._side_stream()
        streams = {MAIN: (torch.cuda.current_stream(), st), SIDE: (side, C.c_void_p(side.cuda_stream))}
        events = EventJoiner(self._ev, streams)
        return events if self.handoff is None else FlagJoiner(self, events, main_wait)

    def _walk(self, rows, joiner, **extra):
        """Walk schedule rows with a joiner; extra: run-time keyword arguments per piece."""
        def run(s, sig):
            kw = dict(s.args, **extra.get(s.piece, {}))
            if sig is not None:
                kw['sig'] = sig
            getattr(self, s.piece)(joiner.streams[s.stream][1], **kw)
        walk(rows, joiner, run)

    # The step's pieces, per stream, between its cross-stream dependencies (gpi.schedule says which follows
    # which; the joiners realise the edges between them).
    def forward_a(self, st, zero_gacc=True, zero_scratch=True):
        """Main stream, up to the ROM fork: scratch / accumulator reset, encoder forward, head forward."""
        if zero_scratch:
            self.ws.zero_scratch()
        if zero_gacc:
            self.flat.gacc.zero_()
        if self.ep is not None:
            self._codec(True, self.enc_descs, 0, self.n_enc_conv, self.ectx, st, 'encoder forward')
        if not self.armortized and self.B_u > 0:
            # q_z['unsupervised'] rows as the "encoder" outputs of the head's first segment
            # (torch copies on the current stream, which the launches use)
            self.ws.view(self.hb['zmu'], self.B_u, self.dz).copy_(self.q_unsup._mean.detach())
            self.ws.view(self.hb['zls'], self.B_u, self.dz).copy_(self.q_unsup._logsigma.detach())
        head_forward(self.head, self.flat, self.ws, st)

    def forward_b(self, st, sig=None):
        """Main stream: decoder forward and its fused output conv (forward + loss + backward); sig: hand-off
        flag its first launch signals."""
        self._codec(True, self.dec_descs, 0, self.n_dec_sep, self.dctx, st, 'decoder forward', sig=sig)
        if self.n_dec_sep < len(self.dec_descs):
            _run(_lib().gpi_conv_loss_fused, C.byref(self.dec_descs[self.n_dec_sep]), C.byref(self.dctx), st,
                 what='decoder output conv (forward + loss + backward)')

    def running_now(self, st):
        """Main stream, end of the forward: the BN running statistics (running='now')."""
        self.running.launch(st)

    def rom_side(self, sst):
        """Side stream: the ROM solves (after the head forward); with the MLP effective-property map its
        forward (mu_X, X~, logL_X, entropy from the head's z) ahead of them."""
        if self.side_pre is not None:
            self.side_pre(sst)
        if self.gpm is not None:
            self._gp_forward(sst)
        for r in self.roms:
            _run(_lib().gpi_rom, C.byref(r), sst, what='rom')

    def backward_a(self, st, split):
        """Main stream: decoder backward and the head backward (encoder samples only when split:
        the variational samples' need the ROM adjoint and follow it on the side stream)."""
        self._codec(False, self.dec_descs, 0, self.n_dec_sep, self.dctx, st, 'decoder backward')
        if split:
            self._head_part(L.HEAD_PART_ENC, st)
        else:
            if self.gpm is not None:
                self._gp_backward(st)
            head_backward(self.head, self.flat, self.ws, st)
        if not self.armortized and self.B_u > 0:
            # d/dmu, d/dlogsigma of q_z['unsupervised'] (written by the head for its first segment)
            n = self.B_u * self.dz
            for src, q in (('dzmu', self.q_unsup._mean), ('dzls', self.q_unsup._logsigma)):
                o = self.flat.offset(q)
                self.flat.gacc[o:o + n].add_(self.ws.view(self.hb[src], n).double())

    def backward_b(self, st, sig=None):
        """Main stream: every encoder conv's backward but the input conv's (reverse order); sig: hand-off
        flag its first launch signals."""
        if self.ep is not None and self.n_enc_conv > 1:
            self._codec(False, self.enc_descs, 1, self.n_enc_conv, self.ectx, st, 'encoder backward', sig=sig)
        elif sig is not None:
            self._signal(sig, st)

    def backward_c(self, st, enc_split, sig=None):
        """Main stream: the input conv's backward (weight gradient only) and the encoder slab
        reduction (its own slabs only when enc_split: the side stream reduces the rest); sig: hand-off
        flag the input conv's launch signals."""
        if self.ep is None:
            return
        if self.bn_sync is not None and self.enc_descs[0].gout_mode == 0:
            self._sync_stats(self.enc_descs[0].out_stat, self.enc_descs[0].cout, 2, 'enc')
        if sig is not None:
            _run(_lib().gpi_conv_backward_sig, C.byref(self.enc_descs[0]), C.byref(self.ectx), *self._sig_args(sig),
                 st, what='In_conv backward')
        else:
            _run(_lib().gpi_conv_backward, C.byref(self.enc_descs[0]), C.byref(self.ectx), st,
                 what='In_conv backward')
        run_reduce(self.reduce_enc[:self.n_reduce_in] if enc_split else self.reduce_enc, self.ws, self.flat, st)

    def backward_side_a(self, sst, split, rom=False, running=False, side_extra=None):
        """Side stream, after the decoder backward: the deferred ROM (rom), the variational samples' head
        backward (split), the decoder slab reduction, the deferred BN running statistics (running), the dense
        weight GEMM and side_extra."""
        if rom:
            self.rom_side(sst)
        if split:
            if self.gpm is not None:
                self._gp_backward(sst)          # needs the ROM adjoint, as the head's variational half
            self._head_part(L.HEAD_PART_Q, sst)
        run_reduce(self.reduce_dec, self.ws, self.flat, sst)
        if running:
            self.running.launch(sst)
        if len(self.gemm_items):
            outer_gemm(self.gemm_items, self.flat, self.ws, sst)
        if side_extra is not None:
            side_extra(sst)

    def backward_side_b(self, sst):
        """Side stream, after backward_b: the encoder slab reduction but the input conv's."""
        run_reduce(self.reduce_enc[self.n_reduce_in:], self.ws, self.flat, sst)

    # ------------------------------------------------------------------ SyncBN (optional)
    def set_sync_bn(self, allreduce, world, exchange=None):
        """SyncBN mode (the exact-parity alternative to replica-BN): every BN
        layer normalises over the union of the ranks' batches of its codec call, as the reference does
        over its one process's batch (codec.py:164-173 in train mode).  allreduce(t): in-place SUM
        over the ranks.  After each producing conv the fp64 channel sums {sum x, sum x^2} of its output
        are all-reduced (forward), and before each conv whose output feeds a BN the BN-backward sums
        {sum S, sum S x-hat} of that output (backward) -- once per channel and phase.  The kernels
        divide a sum by their own per-rank count n_r of the codec call's BN group, so the all-reduced
        sum is scaled by n_r / N (N = the group's count over all ranks, all-reduced once here): the
        global means for any per-rank batch sizes.  Every rank must run the same BN groups (a term
        with samples on some ranks only is refused).  The codec launches then go one by one (host
        hook between them); running_var's Bessel factor keeps the per-rank count (N/(N-1) for
        N = per-rank samples x pixels, >= 16384 here: a <1e-4 relative difference in the running
        buffer only).  exchange: a gpi.peer.PeerExchange -- every seam in ONE launch through the ranks'
        IPC-mapped buffers (gpi_bn_exchange GPI_BNX_PEER) instead of fold / allreduce / unfold."""
        # per-group sample counts: the encoder call (group 0), then the decoder's groups in order, and
        # the term presence flags (B_u, N_s, N_vo > 0), all summed over the ranks in ONE collective
        enc_n = [self.B_u if self.ep is not None else 0]
        local = enc_n + list(self.dec_sizes) + [0] * (L.GPI_MAX_GROUPS - len(self.dec_sizes))
        present = [float(n > 0) for n in (self.B_u, self.N_s, self.N_vo)]
        t = torch.tensor([float(n) for n in local] + present, dtype=torch.float64, device=self.flat.P.device)
        allreduce(t)
        tot = t.cpu().tolist()
        if any(abs(p * world - s) > 0.5 for p, s in zip(present, tot[len(local):])):
            raise ValueError('SyncBN: every rank must run the same ELBO terms (B_u / N_s / N_vo > 0 on all or '
                             'none of the ranks); got %s of %d ranks' % (tot[len(local):], world))
        fac = [(n / g if g > 0 else 0.0) for n, g in zip(local, tot[:len(local)])]
        dev = self.flat.P.device
        # scale per (program, group): [GPI_MAX_GROUPS] for the encoder's and the decoder's stat slots
        self.bn_scale = {'enc': torch.tensor([fac[0]] + [0.0] * (L.GPI_MAX_GROUPS - 1), dtype=torch.float64,
                                             device=dev).view(-1, 1, 1),
                         'dec': torch.tensor(fac[1:1 + L.GPI_MAX_GROUPS], dtype=torch.float64,
                                             device=dev).view(-1, 1, 1)}
        self.bn_global_counts = {'enc': tot[0], 'dec': tot[1:1 + len(self.dec_sizes)]}
        self.bn_sync = allreduce
        self.bn_world = int(world)
        self.bn_exchange = exchange
        self._bnx_msg = torch.zeros(L.GPI_BNX_MSG, dtype=torch.float64, device=dev)

    def _stats_view(self):
        R, G = L.GPI_REPLICAS, L.GPI_MAX_GROUPS
        o = N_TERMS * R
        return self.ws.t_scr[o:o + R * G * self.ws.n_stats * 4].view(R, G, self.ws.n_stats, 4)

    def _sync_stats(self, stat0, n, f0, kind):
        """All-reduce the replica-folded sums of stat slots [stat0, stat0 + n), fields f0, f0 + 1, scaled
        per BN group by n_rank / N_global (set_sync_bn), back into replica 0: gpi_bn_exchange FOLD, the
        collective on the [groups, n, 2] message, UNFOLD -- or the one-shot peer form (one launch)."""
        lib = _lib()
        d = L.BnExchangeDesc(stats=self.ws.stats_ptr.value, n_stats=self.ws.n_stats, stat0=stat0, n=n, f0=f0,
                             scale=self.bn_scale[kind].data_ptr(), msg=self._bnx_msg.data_ptr())
        st = L.stream_handle()
        if self.bn_exchange is not None:
            self.bn_exchange.fill(d)
            _run(lib.gpi_bn_exchange, C.byref(d), st, what='SyncBN peer exchange')
            return
        d.mode = L.BNX_FOLD
        _run(lib.gpi_bn_exchange, C.byref(d), st, what='SyncBN fold')
        self.bn_sync(self._bnx_msg[:L.GPI_MAX_GROUPS * n * 2])
        d.mode = L.BNX_UNFOLD
        _run(lib.gpi_bn_exchange, C.byref(d), st, what='SyncBN unfold')

    def _codec_kind(self, descs):
        return 'enc' if self.ep is not None and descs is self.enc_descs else 'dec'

    def _codec(self, fwd, descs, i0, i1, ctx, st, what, sig=None):
        """The convs descs[i0] .. descs[i1 - 1] forward (fwd), or descs[i1 - 1] down to descs[i0] backward
        (gpi_codec_backward's order); sig: hand-off flag the first launch signals (the *_sig entry points)."""
        lib = _lib()
        sa = self._sig_args(sig) if sig is not None else (None, None)
        if i1 <= i0:
            if sig is not None:
                self._signal(sig, st)
            return
        if self.bn_sync is None:
            ptr = C.cast(C.byref(descs, i0 * C.sizeof(L.ConvDesc)), C.POINTER(L.ConvDesc))
            _run(lib.gpi_codec_forward_sig if fwd else lib.gpi_codec_backward_sig, ptr, i1 - i0, C.byref(ctx), *sa,
                 st, what=what)
            return
        kind = self._codec_kind(descs)
        order = range(i0, i1) if fwd else range(i1 - 1, i0 - 1, -1)
        for i in order:
            d = descs[i]
            if not fwd and d.gout_mode == 0:          # its output feeds a BN: that BN's backward sums are complete
                self._sync_stats(d.out_stat, d.cout, 2, kind)
            _run(lib.gpi_conv_forward_sig if fwd else lib.gpi_conv_backward_sig, C.byref(d), C.byref(ctx),
                 *(sa if i == order[0] else (None, None)), st, what=what)
            if fwd and d.epilogue == L.EPI_STORE_STATS and d.out_stat >= 0:
                self._sync_stats(d.out_stat, d.cout, 0, kind)

    def _side_stream(self):
        """The side stream and, with it, the events of the schedule's edges (and of the step gate)."""
        if self._side is None:
            self._side = torch.cuda.Stream(device=torch.cuda.current_stream().device)
            self._ev = {k: torch.cuda.Event() for k in (E_ROM, E_DEC, E_ENC, E_SIDE, E_VALUE, 'start')}
        return self._side

    def _check_rom_written(self):
        if self._rom_deferred:
            # GPI_ROM_AT=backward with compute_value=False: the ROM (and its log-likelihood terms) runs
            # with the backward's side work, so the terms are not written until backward() is enqueued
            raise RuntimeError('ElboEngine: the ROM log-likelihood is deferred to the backward '
                               '(rom_at="backward"); read the ELBO terms after backward()')

    def elbo_value(self, terms=None):
        """0-d ELBO from the term accumulators (or from a saved copy ``terms`` [N_TERMS * R])."""
        if terms is None:
            self._check_rom_written()
        t = self.ws.terms if terms is None else terms.view(N_TERMS, R).sum(1)
        su, ss, sv = self.su, self.ss, self.sv
        val = t.new_zeros(())
        if self.B_u > 0:
            val = val + su * (t[T_LX0] - (t[T_KL_ENC] if self.armortized else t[T_KL_Q]))
        if self.N_s > 0:
            v = t[T_LX0 + self.g_sup] + t[T_LOGL_Y] - t[T_KL_Q]
            if not self.lockx:
                v = v + t[T_LOGL_X] + t[T_ENT] + self.N_s * ENT_CONST
            val = val + ss * v
        if self.N_vo > 0:
            v = t[T_LX0 + self.g_vo] - t[T_KL_Q2]
            if not self.vo_holdoff:
                v = v + t[T_LOGL_Y2]
                if not self.lockx:
                    v = v + t[T_LOGL_X2] + t[T_ENT2] + self.N_vo * ENT_CONST
            val = val + sv * v
        return val.to(torch.float32)

    def terms(self, terms=None):
        """Dictionary of the individual ELBO terms (host sync), from the term accumulators or from a saved
        copy ``terms`` [N_TERMS * R] (the fused step's, whose epilogue clears the accumulators)."""
        if terms is None:
            self._check_rom_written()
        t = (self.ws.terms if terms is None else terms.view(N_TERMS, R).sum(1)).cpu()
        out = {}
        gi = 0
        if self.B_u > 0:
            if self.armortized:
                out['ARM_unsupervised_logL_x'] = float(t[T_LX0])
                out['ARM_unsupervised_DKL_z'] = float(t[T_KL_ENC])
            else:
                out['unsupervised_logL_x'] = float(t[T_LX0])
                out['unsupervised_DKL_z'] = float(t[T_KL_Q])
            gi = 1
        if self.N_s > 0:
            out['supervised_logL_x'] = float(t[T_LX0 + gi])
            out['supervised_logL_y'] = float(t[T_LOGL_Y])
            out['supervised_DKL_z'] = float(t[T_KL_Q])
            if not self.lockx:
                out['supervised_logL_X'] = float(t[T_LOGL_X])
                out['supervised_entropy_X'] = float(t[T_ENT]) + self.N_s * ENT_CONST
        if self.N_vo > 0:
            out['vo_logL_x'] = float(t[T_LX0 + self.g_vo])
            out['vo_DKL'] = float(t[T_KL_Q2])
            if not self.vo_holdoff:
                out['vo_logL_y'] = float(t[T_LOGL_Y2])
                if not self.lockx:
                    out['vo_logL_X'] = float(t[T_LOGL_X2])
                    out['vo_entropy'] = float(t[T_ENT2]) + self.N_vo * ENT_CONST
        return out

    def finalize(self, out, accumulate=False, step=None, stream=None, zero_acc=False):
        st = stream if stream is not None else L.stream_handle()
        flags = (L.FINALIZE_ACCUMULATE if accumulate else 0) | (L.FINALIZE_ZERO if zero_acc else 0)
        _run(_lib().gpi_grad_finalize, C.c_void_p(self.flat.gacc.data_ptr()), C.c_void_p(out.data_ptr()),
             self.flat.numel, flags, C.c_void_p(step.data_ptr()) if step is not None else None, st,
             what='grad finalize')

    def check_flag(self):
        """Lazy replacement of ROM.py:75's per-step host sync."""
        if int(self.ws.t_flag[0].item()) != 0:
            raise ValueError('At least one of the conductivity values supplied to the ROM was smaller than 1e-12')


# ==========================================================================
# standalone operators (CNNEncoder.forward, CNNDecoder.forward, ROM, CGR)
# ==========================================================================
class EncoderEngine(object):
    """CNNEncoder.forward (Encoder.py:191-196): x -> (mean, logsigma) and its backward."""

    def __init__(self, enc, flat, B):
        off = codec_setup(self, 'enc', enc, flat, B)
        self.reduce_items = self.p.reduce_items(off)
        self.gemm_items = gemm_array(encoder_head_gemms(self.head, self.hb, self.B))
        self.running = BnRunning([(self.p, enc, [(0, self.B)])], self.ws, flat.P.device)

    def forward(self, x, dropout=None, seed=0):
        """dropout: optional injected channel scales {conv name: [B, cout]} (else drawn, seed)."""
        L.require_device(x)
        x = x.contiguous().float()
        self._x = x
        self.ctx.ext_in = x.data_ptr()
        self.ctx.ext_idx = None
        lib, st = _lib(), L.stream_handle()
        if self.p.drop_numel:
            if dropout is not None:
                inject_dropout(dropout_views(self.ws, (('enc', self.p, self.B),)), {'enc': dropout})
            else:
                draw_dropout(self.ws, (self.p,), st, seed)
        self.ws.zero_scratch()
        _run(lib.gpi_codec_forward, self.descs, len(self.descs), C.byref(self.ctx), st, what='encoder forward')
        self.running.launch(st)
        head_forward(self.head, self.flat, self.ws, st)
        return (self.ws.view(self.hb['zmu'], self.B, self.dz).clone(),
                self.ws.view(self.hb['zls'], self.B, self.dz).clone())

    def backward(self, dmu, dls):
        st = L.stream_handle()
        self.ws.view(self.hb['gz'], self.B, self.dz).copy_(dmu)
        self.ws.view(self.hb['dzls'], self.B, self.dz).copy_(dls)
        self.flat.gacc.zero_()
        head_backward(self.head, self.flat, self.ws, st)
        _run(_lib().gpi_codec_backward, self.descs, len(self.descs), C.byref(self.ctx), st, what='encoder backward')
        run_reduce(self.reduce_items, self.ws, self.flat, st)
        outer_gemm(self.gemm_items, self.flat, self.ws, st)


class DecoderEngine(object):
    """CNNDecoder.forward (Decoder.py:288-305): z -> (mean, logsigma) [B, H, W] and its backward."""

    def __init__(self, dec, flat, B):
        off = codec_setup(self, 'dec', dec, flat, B)
        self.reduce_items = self.p.reduce_items(off)
        self.gemm_items = gemm_array(decoder_latent_gemms(self.head, self.hb, self.B))
        o = self.p.output
        self.out_shape = (self.B, o.C, o.H, o.W)
        self.running = BnRunning([(self.p, dec, [(0, self.B)])], self.ws, flat.P.device)

    def forward(self, z, dropout=None, seed=0):
        """dropout: optional injected channel scales {conv name: [B, cout]} (else drawn, seed)."""
        L.require_device(z)
        lib, st = _lib(), L.stream_handle()
        self.ws.view(self.hb['z'], self.B, self.dz).copy_(z)
        if self.p.drop_numel:
            if dropout is not None:
                inject_dropout(dropout_views(self.ws, (('dec', self.p, self.B),)), {'dec': dropout})
            else:
                draw_dropout(self.ws, (self.p,), st, seed)
        self.ws.zero_scratch()
        head_forward(self.head, self.flat, self.ws, st, what='latent map')
        _run(lib.gpi_codec_forward, self.descs, len(self.descs), C.byref(self.ctx), st, what='decoder forward')
        self.running.launch(st)
        return self.ws.view(self.p.output.off, *self.out_shape).clone()

    def backward(self, dout):
        st = L.stream_handle()
        self.ws.view(self.p.output.s_off, *self.out_shape).copy_(dout)
        self.flat.gacc.zero_()
        _run(_lib().gpi_codec_backward, self.descs, len(self.descs), C.byref(self.ctx), st, what='decoder backward')
        head_backward(self.head, self.flat, self.ws, st, what='latent map bwd')
        run_reduce(self.reduce_items, self.ws, self.flat, st)
        outer_gemm(self.gemm_items, self.flat, self.ws, st)
        return self.ws.view(self.hb['dzmu'], self.B, self.dz).clone()


def ROM_NN(nc):
    """Number of coarse nodes of the nc x nc ROM mesh."""
    return (nc + 1) ** 2


def rom_call(nc, refine, x, F, input_kappa, mode, mu_y=None, uc=None, dmu=None, duc=None, gx=None, Y=None,
             logsig_y=None, gacc_logsig=None, loss_acc=None, flag=None, loss_scale=1.0, gx_accumulate=False,
             gls_part=None, y_weight=None, yw_stride=None):
    """Thin launcher of gpi_rom for the standalone ROM / ReducedOrderModelOperator.  y_weight (LOGLIK): fp32
    observation weights, [d_y] shared or [n, d_y] (yw_stride overrides the stride taken from its shape)."""
    for t in (x, F):
        L.require_device(t)
    r = L.RomDesc()
    r.nc, r.refine, r.n, r.mode, r.input_kappa = nc, refine, x.shape[0], mode, 1 if input_kappa else 0
    r.x, r.x_stride, r.F = x.data_ptr(), x.stride(0), F.data_ptr()
    p = lambda t: t.data_ptr() if t is not None else None
    r.mu_y, r.uc, r.dmu, r.duc, r.gx, r.Y, r.logsig_y = p(mu_y), p(uc), p(dmu), p(duc), p(gx), p(Y), p(logsig_y)
    r.gx_stride = gx.stride(0) if gx is not None else 0
    r.gacc_logsig, r.loss_acc, r.flag, r.gls_part = p(gacc_logsig), p(loss_acc), p(flag), p(gls_part)
    r.loss_scale, r.gx_accumulate = loss_scale, 1 if gx_accumulate else 0
    if y_weight is not None:
        L.require_device(y_weight)
        r.y_weight = y_weight.data_ptr()
        r.yw_stride = (y_weight.stride(0) if y_weight.dim() == 2 else 0) if yw_stride is None else yw_stride
    _run(_lib().gpi_rom, C.byref(r), L.stream_handle(), what='rom')


def cgr_residual(logkappa_img, y, bc, nc, flux=False):
    """W^T [K(kappa) yhat]_free for a batch of fields -> [N, (nc+1)^2]; flux=True also returns the
    flux-constraint residual Gamma_fc y [N, 2 nc^2] of the same pass (flux.py:81-158, alpha = 0)."""
    for t in (logkappa_img, y, bc):
        L.require_device(t)
    N, n = logkappa_img.shape[0], logkappa_img.shape[-1]
    r = torch.empty(N, (nc + 1) ** 2, dtype=torch.float32, device=y.device)
    d = L.ResidualDesc()
    lk, yy, bb = logkappa_img.contiguous().float(), y.contiguous().float(), bc.contiguous().float()
    d.n_fine, d.nc, d.n = n, nc, N
    rf = torch.empty(N, 2 * nc * nc, dtype=torch.float32, device=y.device) if flux else None
    d.logkappa, d.y, d.bc, d.r = lk.data_ptr(), yy.data_ptr(), bb.data_ptr(), r.data_ptr()
    d.r_flux = rf.data_ptr() if flux else None
    _run(_lib().gpi_cgr_residual, C.byref(d), L.stream_handle(), what='cgr residual')
    return (r, rf) if flux else r
