"""Inference (eval mode): running-statistic BatchNorm codec engines and the surrogate predictor.

EvalEncoderEngine / EvalDecoderEngine -- CNNEncoder / CNNDecoder forward of a module in ``.eval()``:
    BatchNorm2d normalises with its running statistics, Dropout2d is the identity, nothing is
    written back to the module.  The conv kernels are the training path's, unchanged: per call
        seed (gpi_bn_eval_seed) -> gpi_codec_forward -> head forward            (encoder)
        latent map -> seed -> gpi_codec_forward                                (decoder)
    The seed writes, for every BN layer, the fp64 (sum, sum^2) records whose mean / biased variance
    are the layer's running statistics, so the forward kernels' relu(BN)-on-load applies the eval
    affine map.  It runs on every call: load_state_dict, training steps and the prediction-ensemble
    fold all write the running buffers in place.  Every BN layer has its own records (plan.layout
    eval_mode).  No statistics epilogue, no running update, no dropout draw, no scratch zero-fill, no
    backward buffers; the outputs carry no autograd graph.

SurrogatePredictor -- the deployable x -> y map of a DiscriminativeModel (or of a GenerativeModel and
    its encoder) for a fixed batch size: encoder (eval) -> head -> gp mean (gpi_affine, no noise drawn
    or read) -> gpi_rom FORWARD, over static buffers, optionally replayed as one HIP graph.
"""
import ctypes as C

import torch

from . import _lib as L
from .engine import codec_setup, head_forward, rom_call, _run, _lib, ROM_NN, gp_linears, check_gp_hidden


class BnEvalSeed(object):
    """The gpi_bn_eval_seed items of one eval program: one per BN-consuming conv (its own stat range)."""

    def __init__(self, prog, module, B, ws, device):
        self.ws, self.device, self.B = ws, device, int(B)
        self.layers = [(op, module.get_submodule(op.bn)) for op in prog.ops if op.bn is not None]
        self.max_ch = max([op.cin for op, _ in self.layers] + [1])
        self.n = len(self.layers)
        self._ptrs = None
        self.refresh()

    def _buffers(self):
        out = []
        for op, bn in self.layers:
            rm, rv = bn.running_mean, bn.running_var
            if rm is None or rv is None:
                raise L.NativeError('eval-mode forward needs running statistics: %s has track_running_stats=False'
                                    % op.bn)
            for t in (rm, rv):
                L.require_device(t)
                if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != op.cin:
                    raise L.NativeError('running statistics of %s: expected %d contiguous fp32 values' % (op.bn, op.cin))
            if abs(bn.eps - 1e-5) > 1e-12:
                raise L.NativeError('%s: only eps = 1e-5 is supported' % op.bn)
            out.append((rm, rv))
        return out

    def refresh(self):
        """(Re)build the device item list when a running buffer is a new tensor (module.to(), a buffer
        assignment); in-place writes (load_state_dict, training, the ensemble fold) need nothing: the
        seed kernel reads the buffers at every call."""
        bufs = self._buffers()
        ptrs = tuple(t.data_ptr() for pair in bufs for t in pair)
        if ptrs == self._ptrs or not self.n:
            return
        items = []
        for (op, _), (rm, rv) in zip(self.layers, bufs):
            it = L.BnEvalItem()
            it.stat, it.channels = op.desc.in_stat, op.cin
            it.count = float(self.B * op.src.H * op.src.W)
            it.running_mean, it.running_var = rm.data_ptr(), rv.data_ptr()
            items.append(it)
        raw = bytearray(bytes((L.BnEvalItem * self.n)(*items)))
        self.dev = torch.frombuffer(raw, dtype=torch.uint8).to(self.device)
        self._ptrs = ptrs

    def launch(self, stream):
        if self.n:
            _run(_lib().gpi_bn_eval_seed, C.c_void_p(self.dev.data_ptr()), self.n, self.max_ch, self.ws.stats_ptr,
                 self.ws.n_stats, stream, what='bn eval seed')


class EvalEncoderEngine(object):
    """CNNEncoder.forward in eval mode: x -> (mean, logsigma), forward only."""
    mode = 'eval'

    def __init__(self, enc, flat, B):
        codec_setup(self, 'enc', enc, flat, B, train=False)
        ws, hb, dz, dev = self.ws, self.hb, self.dz, flat.P.device
        self.seed = BnEvalSeed(self.p, enc, self.B, ws, dev)
        self.mu = ws.view(hb['zmu'], self.B, dz)
        self.logsigma = ws.view(hb['zls'], self.B, dz)

    def launch(self, x, st):
        """Enqueue the forward on stream handle st for the contiguous fp32 device tensor x [B, 1, H, W];
        the results land in self.mu / self.logsigma (workspace views, overwritten by the next call)."""
        self._x = x
        self.ctx.ext_in = x.data_ptr()
        self.ctx.ext_idx = None
        self.seed.launch(st)
        _run(_lib().gpi_codec_forward, self.descs, len(self.descs), C.byref(self.ctx), st,
             what='encoder eval forward')
        head_forward(self.head, self.flat, self.ws, st)

    def forward(self, x):
        L.require_device(x)
        x = x.contiguous().float()
        if x.numel() != self.B * self.p.input.per_sample:
            raise ValueError('encoder input %s does not match batch %d of %s images'
                             % (tuple(x.shape), self.B, (self.p.input.H, self.p.input.W)))
        self.seed.refresh()
        self.launch(x, L.stream_handle())
        return self.mu.clone(), self.logsigma.clone()


class EvalDecoderEngine(object):
    """CNNDecoder.forward in eval mode: z -> (mean, logsigma) [B, 2, H, W], or the probability image
    [B, 1, H, W] of a binary decoder (the sigmoid of the kernels' logit image), or the mean image
    [B, 1, H, W] of a homoscedastic decoder (CNNDecoder.forward expands its log-sigma plane beside it, on the
    host side: the plane is a parameter, not a kernel output); forward only."""
    mode = 'eval'

    def __init__(self, dec, flat, B):
        codec_setup(self, 'dec', dec, flat, B, train=False)
        self.binary = bool(getattr(dec, '_binary', False))
        o = self.p.output
        self.out_shape = (self.B, o.C, o.H, o.W)
        self.seed = BnEvalSeed(self.p, dec, self.B, self.ws, flat.P.device)

    def forward(self, z):
        L.require_device(z)
        st = L.stream_handle()
        self.seed.refresh()
        self.ws.view(self.hb['z'], self.B, self.dz).copy_(z)
        head_forward(self.head, self.flat, self.ws, st, what='latent map')
        self.seed.launch(st)
        _run(_lib().gpi_codec_forward, self.descs, len(self.descs), C.byref(self.ctx), st, what='decoder eval forward')
        out = self.ws.view(self.p.output.off, *self.out_shape)
        return torch.sigmoid(out) if self.binary else out.clone()


# ---------------------------------------------------------------- surrogate predictor
class _PredictiveModel(object):
    """The attributes predictive_y reads (gp with .fc / .independent_X / .logsigmas_X, g)."""

    class _DeterministicGp(object):
        independent_X = False

        def __init__(self, fc):
            self.fc = fc

    def __init__(self, gp, g):
        self.gp = gp if hasattr(gp, 'fc') else self._DeterministicGp(gp)
        self.g = g


class SurrogatePredictor(object):
    """x -> y mean of the trained surrogate for a fixed batch size B, over static buffers.

        p = SurrogatePredictor(disc, B)            # a DiscriminativeModel with its encoder
        p = SurrogatePredictor(model, B)           # a GenerativeModel (its registered encoder, gp, g)
        y = p.predict(X, F)                        # [B, d_y]; a view of the static output
        p.capture(); p.X.copy_(X2); p.F.copy_(F2); y = p.replay()

    The encoder always runs its eval-mode engine here (running-statistic BN, no dropout), whatever
    its .training flag says.  predict draws and reads no noise."""

    def __init__(self, model, B, encoder=None):
        from .native import module_flat
        if hasattr(model, '_encoder'):          # DiscriminativeModel
            enc, gp, g = (encoder if encoder is not None else model._encoder), model._gp, model._g
        else:                                   # GenerativeModel
            enc, gp, g = (encoder if encoder is not None else model.encoder), model.gp, model.g
        if enc is None:
            raise ValueError('SurrogatePredictor needs an encoder (the model has none registered)')
        self.B = int(B)
        self.enc, self.gp, self.g = enc, gp, g
        self.fc = gp.fc if hasattr(gp, 'fc') else gp
        # the map's nn.Linear layers: one (gpi_affine) or the MLP's fc1 .. fc{L+1} (gpi_gpmlp_sample, mean only)
        self.linears = gp_linears(self.fc)
        check_gp_hidden(len(self.linears) - 1)
        dev = self.linears[0].weight.device
        L.require_device(self.linears[0].weight)
        self.device = dev
        flat = module_flat(enc, dev)
        self.flat = flat
        self.engine = EvalEncoderEngine(enc, flat, self.B)
        rom = g.rom
        self.nc, self.refine = rom.nc, rom.refine
        self.d_x, self.d_y, self.dz = g.dim_effective_property, g.dim_out, self.engine.dz
        if (self.linears[0].in_features, self.linears[-1].out_features) != (self.dz, self.d_x):
            raise ValueError('gp map %s does not take the encoder mean [%d] to the ROM input [%d]'
                             % ((self.linears[0].in_features, self.linears[-1].out_features), self.dz, self.d_x))
        inp = self.engine.p.input
        self.X = torch.zeros(self.B, 1, inp.H, inp.W, dtype=torch.float32, device=dev)
        self.F = torch.zeros(self.B, ROM_NN(self.nc), dtype=torch.float32, device=dev)
        self.x_eff = torch.zeros(self.B, self.d_x, dtype=torch.float32, device=dev)
        self.y = torch.zeros(self.B, self.d_y, dtype=torch.float32, device=dev)
        self.flag = torch.zeros(1, dtype=torch.int32, device=dev)
        self.graph = None

    # ------------------------------------------------------------------
    def _launch(self):
        st = L.stream_handle()
        self.engine.launch(self.X, st)
        if len(self.linears) > 1:
            from .predictive import gp_mlp_sample
            # (the launch reads the parameters' own storage: _check_params -- run by predict() and, before it bakes
            # the pointers, by capture() -- requires contiguous fp32 weights, for which detach().contiguous() is a
            # view, so nothing the returned keep-alive tuple holds can go away while the modules live)
            gp_mlp_sample(self.linears, self.engine.mu, None, None, self.x_eff, stream=st)
        else:
            w, b = self.fc.weight, self.fc.bias
            _run(_lib().gpi_affine, L.ptr(w), L.ptr(b), L.ptr(self.engine.mu), L.ptr(self.x_eff), self.B, self.d_x,
                 self.dz, st, what='gp mean')
        rom_call(self.nc, self.refine, self.x_eff, self.F, False, L.ROM_FORWARD, mu_y=self.y, flag=self.flag)

    def _check_params(self):
        if not all(self.flat.owns(p) for p in self.enc.parameters()):
            raise L.NativeError('the encoder parameters were re-allocated since this SurrogatePredictor was built '
                                '(module.to() / a new flat buffer): build a new predictor')
        for t in [p for fc in self.linears for p in (fc.weight, fc.bias) if p is not None]:
            if t.dtype != torch.float32 or not t.is_contiguous() or t.device != self.device:
                raise L.NativeError('gp map: contiguous fp32 parameters on %s expected' % self.device)

    def _stage(self, X, F):
        L.require_device(X)
        L.require_device(F)
        if X.numel() != self.X.numel() or F.numel() != self.F.numel():
            raise ValueError('SurrogatePredictor(B=%d): got X %s, F %s' % (self.B, tuple(X.shape), tuple(F.shape)))
        self.X.copy_(X.detach().reshape(self.X.shape))
        self.F.copy_(F.detach().reshape(self.F.shape))

    @torch.no_grad()
    def predict(self, X=None, F=None):
        """y mean [B, d_y] (a view of the static output buffer: clone it to keep it across calls).
        X, F None: run on the current contents of the static buffers self.X / self.F."""
        if X is not None:
            self._stage(X, F)
        self._check_params()
        self.engine.seed.refresh()
        self._launch()
        return self.y

    @torch.no_grad()
    def encode(self, X):
        """Eval-mode encoder (mu, logsigma) [B, d_z] of X (clones)."""
        self.X.copy_(X.detach().reshape(self.X.shape))
        self._check_params()
        self.engine.seed.refresh()
        self.engine.launch(self.X, L.stream_handle())
        return self.engine.mu.clone(), self.engine.logsigma.clone()

    @torch.no_grad()
    def predict_mc(self, X, F, N_mc, eps=None):
        """(mean, std) [B, d_y] of the MC predictive y at the encoder's eval (mu, logsigma)
        (gpi.predictive.predictive_y; eps optionally injects (eps_z, eps_x or None, eps_y))."""
        from .predictive import predictive_y
        mu, ls = self.encode(X)
        Fm = F.detach().reshape(self.F.shape).float().contiguous()
        return predictive_y(_PredictiveModel(self.gp, self.g), mu, ls, Fm, int(N_mc), eps=eps)

    def capture(self):
        """Record predict() on the static buffers as one HIP graph (one stream, no parallel
        branches); replay() then re-runs it on whatever self.X / self.F hold.  The graph holds the
        device pointers of the parameters and running buffers: their in-place updates are picked up,
        re-allocations are not (build a new predictor)."""
        self._check_params()
        self.engine.seed.refresh()
        side = torch.cuda.Stream(device=self.device)
        side.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(side), torch.no_grad():
            self._launch()                      # warm-up outside the capture (lazy module loads)
        torch.cuda.current_stream(self.device).wait_stream(side)
        torch.cuda.synchronize(self.device)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g), torch.no_grad():
            self._launch()
        self.graph = g
        return self

    def replay(self):
        if self.graph is None:
            raise RuntimeError('SurrogatePredictor.replay() before capture()')
        self.graph.replay()
        return self.y

    def check_flag(self):
        """Lazy ROM check (host sync): raises if any effective conductivity was <= 1e-12 since the last check."""
        if int(self.flag.item()) != 0:
            self.flag.zero_()
            raise ValueError('At least one of the conductivity values supplied to the ROM was smaller than 1e-12')
