"""Fused native training step: Trainer.run's loop body (training.py:403-417)
without Python/autograd glue, for production runs and the benchmark.

One step = random armortized subset (utils/data.py:444) + reparametrisation
noise (device Philox) + ELBO forward/backward (ElboEngine) + gradient
finalisation + [one SUM all-reduce of the shared-parameter gradients over
RCCL] + flat Adam (training.py:254,417).  Per-sample variational parameters
(q_z / q_X rows of this rank's labeled samples) are rank-local and never
communicated.  Every launch is stream-ordered with no host synchronisation,
so the whole step can be captured once into a HIP graph and replayed.
"""
import ctypes as C
import os

import torch
import torch.distributed as dist

from . import _lib as L
from . import vo as gvo
from .engine import ElboEngine
from .schedule import MAIN, SIDE, E_ROM, E_DEC, E_ENC, E_SIDE, segments

# Philox sub ids of the virtual-observable targets y ~ N(VO.mean, VO.var) (generative.py:356).  The step's
# draws use sub0 + {1 subset, 2 eps_z, 3 eps_X, 4 / 5 encoder / decoder Dropout2d, 6 y_vo} with sub0 = 0
# for the draws made during a step (for the next one) and sub0 = 100 for the constructor's; the redraw of
# the pending target after a VO update uses VO_REDRAW_SUB, the draws after a hold-off switch sub0 =
# VO_SWITCH_SUB0 -- all at the step's current Philox offset.
VO_Y_SUB = 6
VO_REDRAW_SUB = 206
VO_SWITCH_SUB0 = 300
NO_POSTERIOR = 'the virtual observables have no posterior yet: call update_virtual_observables'


def vo_buffers(vo):
    """The persistent fp32 (mean, logsigma) device buffers of a VO ensemble, which its updates write in place
    (VirtualObservablesEnsemble / EnergyVirtualObservablesEnsemble)."""
    if hasattr(vo, '_mean32'):
        return vo._mean32, vo._logsig32
    return vo.mean32, vo.logsig32


def allreduce_shared(flat, group=None):
    """Data-parallel gradient exchange: ONE SUM all-reduce
    (the ELBO is a sum over samples, normalize=False) of the shared-parameter
    prefix G[:n_shared] of the flat gradient; the per-sample variational rows
    that follow it are rank-owned and never communicated."""
    n = flat.n_shared
    if n > 0:
        dist.all_reduce(flat.G[:n], op=dist.ReduceOp.SUM, group=group)


def l2_segments(model, flat=None):
    """The tensors model.elbo(l2_penalty=) penalises (generative.py:381-385: f.parameters(), then
    encoder.parameters() when the model has an encoder) as rows (name, offset, numel) of the flat parameter
    buffer, in that order.  No device work."""
    flat = flat if flat is not None else model.native_flat()
    rows = []
    for prefix, mod in (('f.', model.f), ('encoder.', getattr(model, 'encoder', None))):
        if mod is not None:
            rows += [(prefix + n, flat.offset(p), p.numel()) for n, p in mod.named_parameters()]
    return rows


def param_norms(desc, stream):
    """One gpi_param_norms launch (the fused step's only call site of the entry point)."""
    L.check(L.lib().gpi_param_norms(C.byref(desc), stream), 'parameter norms')


class FusedAdamSchedule(torch.optim.Optimizer):
    """The learning-rate handle of a FusedElboStep as a torch Optimizer, so that torch LR schedulers
    (and lamp.optimization.LearningScheduleWrapper, lamp/optimization.py:71-93, training.py:452,615)
    drive the fused step's device-resident Adam exactly as they drive torch.optim.Adam: the
    scheduler edits ``param_groups[0]['lr']``; FusedElboStep copies a changed value into the
    device learning rate before its next step (an async fill, no host synchronisation)."""

    def __init__(self, lr, betas, eps):
        super().__init__([torch.zeros(1)], dict(lr=lr, betas=betas, eps=eps))

    def step(self, closure=None):     # the update itself runs inside the fused step
        return None


class FusedElboStep(object):
    """rank / world: data-parallel position.  Every rank holds the same global unlabeled pool and
    draws the same global permutation (``subset_seed``, shared) of which it takes its B_u-slice
    (SURVEY.md section 8e); labeled samples and their q rows are rank-owned; the
    reparametrisation noise uses ``seed`` (per rank).

    X_vo / F_vo (single process only): the virtual-observable term of model.elbo (generative.py:341-392) in
    the step -- a third decoder BN group, the q['vo'] rows as the head's second segment and a second ROM
    launch against targets y ~ N(vo.mean, vo.var), drawn with the step's other noise from the ensemble's
    persistent fp32 buffers (``vo``: model.VO, either ensemble family).  vo_holdoff: the term's logL_x - KL
    part only (training.py:411); set_vo_holdoff switches.  update_virtual_observables is the loop's VO
    update (training.py:407-409).

    l2_penalty: model.elbo's l2_penalty (generative.py:381-385) in the step.  None (the default): no penalty and
    no launch for it.  A number, 0.0 included: elbo() loses l2_penalty * sum of the 2-norms of the decoder's and
    the encoder's parameter tensors (l2_segments; not divided under normalize=True, as in the reference), the
    gradient gains the penalty's, terms() the reference's 'elbo_l2_penalty'.  One gpi_param_norms launch per step
    on the side stream, beside the next step's noise draws; its fp32 gradient is added where the gradient is
    finalised (the step epilogue).  ``l2`` is a device scalar: set_l2_penalty edits it between steps, captured or
    not.  Data parallel: every rank computes the norms and adds the penalty's gradient to the all-reduced
    gradient after the SUM (in the Adam launch, which stores the sum back into flat.G), so it enters once; rank 0
    alone subtracts the penalty in elbo(), so the ranks' values sum to the global objective."""

    def __init__(self, model, X_pool, B_u, X_s=None, Y=None, F=None, lr=1e-2, betas=(0.9, 0.999), eps=1e-8,
                 seed=0, normalize=False, process_group=None, distributed=False, rank=0, world=1, subset_seed=None,
                 graph_allreduce=True, sync_bn=False, bn_exchange='collective', X_vo=None, F_vo=None, vo=None,
                 vo_holdoff=False, l2_penalty=None):
        self.model = model
        self.N_s = 0 if X_s is None else int(X_s.shape[0])
        self.N_vo = 0 if X_vo is None else int(X_vo.shape[0])
        self.B_u = int(B_u)
        self.rank, self.world = int(rank), int(world)
        assert 0 <= self.rank < self.world
        if self.N_vo and self.world > 1:
            # the learnable flux-row precision beta sums over ALL VO samples (update_vo_precision): ranks that
            # each hold a shard of them would need an exchange of those sums, which does not exist
            raise ValueError('FusedElboStep: the virtual-observable term (X_vo) runs in a single process only: '
                             'the VO precision update sums over all VO samples, and no exchange of a per-rank '
                             "shard's sums exists (world = %d)" % self.world)
        self.flat = model.native_flat()
        self.X_vo, self.F_vo = X_vo, F_vo
        self.vo = None
        if self.N_vo:
            self.vo = vo if vo is not None else model.VO
            if self.vo is None or self.vo is not model.VO:
                raise ValueError('FusedElboStep: vo must be the ensemble registered with the model (model.VO): '
                                 'update_virtual_observables updates that one')
            if self.vo.dtype != torch.float32:
                raise L.NativeError('FusedElboStep: the VO ensemble must keep fp32 mean / logsigma buffers')
            self._vo_ptrs = tuple(t.data_ptr() for t in vo_buffers(self.vo))
        self.normalize = normalize
        # partially observed labels: the model's observation weights as they stand now.  The step (and its
        # captured graphs) holds this tensor's address: an in-place edit is seen by the next step, another
        # tensor needs a new step (_check_label_mask).  Data parallel: the labelled shard and its mask are
        # rank-local, nothing is exchanged.
        self._yw = model.label_weights(self.N_s) if self.N_s else None
        if subset_seed is None and self.world > 1 and self.B_u > 0:
            # every rank must draw the SAME global permutation (its B_u-slice of it); the per-rank
            # noise seed would give overlapping / duplicated slices without any error
            raise ValueError('FusedElboStep: world > 1 needs an explicit subset_seed shared by all ranks')
        self.engine = self._new_engine(vo_holdoff)
        # SyncBN: every codec call's BN statistics over the union of the ranks' batches (ElboEngine.set_sync_bn);
        # default replica-BN (per-rank batch statistics, no collective in the codec).  Any distributed world
        # size, 1 included: a one-rank NCCL job runs (and captures) the same per-conv collectives as the
        # 8-GPU one (tools/dist_capture_probe.py --sync-bn)
        # bn_exchange: 'collective' (each seam's message all-reduced over the process group: RCCL in the graph)
        # or 'peer' (the one-shot exchange through the ranks' IPC-mapped buffers, gpi.peer: one launch per
        # seam, any backend, capturable)
        self.sync_bn = bool(sync_bn) and bool(distributed)
        self.pg = process_group
        self.bn_exchange = bn_exchange if self.sync_bn else None
        self.handoff_flags = torch.zeros(8, dtype=torch.int32, device=self.flat.P.device)   # [0..3] flags, [4] error
        self._peer = None
        if self.sync_bn:
            pg = process_group
            if bn_exchange not in ('collective', 'peer'):
                raise ValueError("bn_exchange: 'collective' or 'peer'")
            if bn_exchange == 'peer':
                from .peer import PeerExchange
                self._peer = PeerExchange(pg, err=self.handoff_flags[4:5])
            self._set_sync_bn(self.engine)
        dev = self.flat.P.device
        self.X_pool = X_pool.contiguous().float() if X_pool is not None else None
        self.X_s, self.Y, self.F = X_s, Y, F
        # global subset of world * B_u pool indices; this rank's slice [rank * B_u, (rank + 1) * B_u)
        self.n_sub = self.world * self.B_u
        self.idx = torch.zeros(max(self.n_sub, 1), dtype=torch.int32, device=dev)
        self.rng_off = torch.zeros(1, dtype=torch.int64, device=dev)
        self.step_ctr = torch.zeros(1, dtype=torch.int64, device=dev)
        self.lr = torch.tensor([lr], dtype=torch.float32, device=dev)
        self.optimizer = FusedAdamSchedule(lr, betas, eps)
        self._lr_host = float(lr)
        self.m = torch.zeros_like(self.flat.P)
        self.v = torch.zeros_like(self.flat.P)
        self.seed = int(seed)
        self.subset_seed = int(seed if subset_seed is None else subset_seed)
        self.distributed = distributed
        # RCCL all-reduce captured inside the step's graph (one replay per step, no host hop between
        # the gradient and the update); host-side between two graphs for gloo
        self.graph_allreduce = bool(graph_allreduce)
        self.adam = L.AdamDesc(p=self.flat.P.data_ptr(), g=self.flat.G.data_ptr(), m=self.m.data_ptr(),
                               v=self.v.data_ptr(), n=self.flat.numel, lr=self.lr.data_ptr(),
                               step=self.step_ctr.data_ptr(), beta1=betas[0], beta2=betas[1], eps=eps)
        self.idx_next = torch.zeros_like(self.idx)
        # A/B switch (tools/critpath_probe.py): draw the next step's subset on the side stream ahead of the ROM
        self.subset_early = False
        # captured form: 'streams' (one graph per stream, ordered only by device counters, _capture_streams:
        # no event edge between the streams at all -- 0.5816 / 0.5827 vs 0.5901 / 0.5904 ms per step with
        # 'single', interleaved on one box, r04g), 'single' (one graph spanning both streams, forked and
        # joined by events at its ends) or 'segments' (single-stream graphs joined by events,
        # _capture_segments: each graph boundary leaves the GPU idle ~15 us: 0.673 vs 0.629 ms, r03).
        # The split DP form (host-side all-reduce between two graphs) keeps 'single'.
        # GPI_GRAPH_MODE overrides (A/B runs)
        self.graph_mode = os.environ.get('GPI_GRAPH_MODE', 'streams')
        if self.graph_mode == 'streams' and self.distributed and not (
                self.graph_allreduce and dist.get_backend(self.pg) == dist.Backend.NCCL):
            self.graph_mode = 'single'
        self._bind(self.engine)
        n_pool = self.X_pool.shape[0] if self.X_pool is not None else 0
        if self.B_u and self.n_sub > n_pool:
            raise ValueError('the pool (%d) is smaller than the global armortized batch (%d)' % (n_pool, self.n_sub))
        self.n_pool = n_pool
        self._subset_ws = None
        if self.B_u and n_pool > 16384:
            nb = C.c_int64(0)
            L.check(L.lib().gpi_random_subset_workspace(n_pool, C.byref(nb)), 'random subset workspace')
            self._subset_ws = torch.zeros(nb.value, dtype=torch.uint8, device=dev)
        drop_span = max([(p.drop_numel + 3) // 4 + 1 for p in (self.engine.ep, self.engine.dp)
                         if p is not None and p.drop_numel] or [0])
        # (the span of the step with the VO term active, whichever variant runs: eps_X over N_s + N_vo rows,
        # the y_vo Gaussian rows one counter per element, not one per four)
        self.rng_span = max(n_pool, (self.engine.B * self.engine.dz + 3) // 4 + 1,
                            ((self.N_s + self.N_vo) * self.engine.d_x + 3) // 4 + 1, drop_span,
                            self.N_vo * self.engine.d_y)
        self.adam.rng_offset = self.rng_off.data_ptr()
        self.adam.rng_advance = self.rng_span
        self.last_terms = torch.zeros(L.GPI_REPLICAS * 16, dtype=torch.float64, device=dev)
        self.l2 = None
        if l2_penalty is not None:
            self._build_l2(float(l2_penalty))
        # single-process steps: the epilogue and Adam in one launch (gpi_step_epilogue_adam; nothing
        # runs between the gradient delivery and the update); GPI_FUSED_ADAM=0 keeps two launches
        self.fuse_adam = not self.distributed and os.environ.get('GPI_FUSED_ADAM', '1') != '0'
        self._build_epilogue()
        self.done_ctr = torch.zeros(1, dtype=torch.int32, device=dev)
        # side-stream hand-offs by device flags (gpi_stream_signal / gpi_stream_wait) instead of graph
        # events between the streams; GPI_HANDOFF=events keeps the events (A/B)
        self.handoff = os.environ.get('GPI_HANDOFF', 'flags') if self.graph_mode in ('single', 'streams') \
            else 'events'
        if self.graph_mode == 'streams' and self.handoff != 'flags':
            self.graph_mode = 'single'
        # 'streams': the side stream is gated per step by this counter (no event between the streams), so
        # each stream's part of the step is captured as a graph of its own
        self.side_done = torch.zeros(1, dtype=torch.int64, device=dev)
        self._probed_stream = None
        self.unroll = 1
        self.g_fb_k = self.g_side_k = None
        self._wire_handoff()
        # lazy surfacing of that error word without a host sync: an async copy to pinned memory after
        # a replay, read once its event has completed (at the next step() / run() / check_handoff())
        self._err_host = torch.zeros(1, dtype=torch.int32, pin_memory=True) if dev.type == 'cuda' else None
        self._err_ev = None
        self._err_every = int(os.environ.get('GPI_ERR_CHECK_EVERY', '16'))
        self._n_steps = 0
        self._fb_pending = False
        self.graph = None
        self._one_draw = os.environ.get('GPI_ONE_DRAW', '1') != '0'
        # the first step's noise; every step then draws the next step's during its backward
        self._launch_noise(L.stream_handle(), self.idx, sub0=100)

    # ------------------------------------------------------------------
    def _new_engine(self, vo_holdoff):
        if not self.N_vo:
            return ElboEngine(self.model, self.B_u, self.N_s, normalize=self.normalize, y_weight=self._yw)
        return ElboEngine(self.model, self.B_u, self.N_s, normalize=self.normalize, N_vo=self.N_vo,
                          vo_holdoff=vo_holdoff, y_weight=self._yw)

    def _check_label_mask(self):
        """Raise when the model's label mask is no longer the tensor this step was built on (set, cleared or
        replaced since): the launches read the old one."""
        if not self.N_s:
            return
        now = self.model.label_weights(self.N_s)
        if (now is None) != (self._yw is None) or (now is not None and (
                now.data_ptr() != self._yw.data_ptr() or tuple(now.shape) != tuple(self._yw.shape))):
            raise L.NativeError('FusedElboStep: the model\'s label mask (preprocess_y_fct / set_label_mask) was '
                                'set, cleared or replaced after the step was built; the step (and its captured '
                                'graphs) reads the old one: rebuild the step.  Edit a mask in place instead.')

    def _set_sync_bn(self, engine):
        pg = self.pg
        engine.set_sync_bn(lambda t: dist.all_reduce(t, op=dist.ReduceOp.SUM, group=pg), self.world,
                           exchange=self._peer)

    def _bind(self, engine):
        my_idx = self.idx[self.rank * self.B_u:(self.rank + 1) * self.B_u] if self.B_u else None
        if self.N_vo:
            engine.bind(X_u=self.X_pool, u_index=my_idx, X_s=self.X_s, Y=self.Y, F=self.F, X_vo=self.X_vo,
                        F_vo=self.F_vo)
        else:
            engine.bind(X_u=self.X_pool, u_index=my_idx, X_s=self.X_s, Y=self.Y, F=self.F)

    def _build_l2(self, l2_penalty):
        """The penalty's buffers and its launch descriptor.  pen_grad is dense over the flat prefix that holds
        the penalised tensors and is written at their elements only: the zeros between them stay."""
        dev = self.flat.P.device
        rows = l2_segments(self.model, self.flat)
        if not rows:
            raise ValueError('FusedElboStep: l2_penalty without a parameter to penalise')
        table = [v for _, o, n in rows for v in (o, n)]
        self.pen_n = max(o + n for _, o, n in rows)
        assert self.pen_n <= self.flat.n_shared
        self._l2_seg_host = (C.c_int64 * len(table))(*table)
        self.l2_seg = torch.tensor(table, dtype=torch.int64, device=dev)
        self.l2 = torch.tensor([l2_penalty], dtype=torch.float32, device=dev)
        self.pen_grad = torch.zeros(self.pen_n, dtype=torch.float32, device=dev)
        self.l2_norms = torch.zeros(len(rows), dtype=torch.float64, device=dev)
        self.l2_pen = torch.zeros(2, dtype=torch.float64, device=dev)      # {pen, l2 * pen} of the running step
        self.last_pen = torch.zeros(2, dtype=torch.float64, device=dev)    # ... of the last completed step
        self.l2_done = torch.zeros(1, dtype=torch.int32, device=dev)
        self.norms_desc = L.ParamNormsDesc(p=self.flat.P.data_ptr(), seg=self.l2_seg.data_ptr(),
                                           seg_host=C.addressof(self._l2_seg_host), n_seg=len(rows),
                                           pen_n=self.pen_n, lam=self.l2.data_ptr(), norms=self.l2_norms.data_ptr(),
                                           pen=self.l2_pen.data_ptr(), pen_grad=self.pen_grad.data_ptr(),
                                           done=self.l2_done.data_ptr())

    def set_l2_penalty(self, value):
        """Change the penalty's factor in place (an async fill, valid between steps; a captured step reads the
        device scalar).  Switching between None and a number needs a new step."""
        if self.l2 is None:
            raise L.NativeError('FusedElboStep.set_l2_penalty: the step was built with l2_penalty=None')
        self.l2.fill_(float(value))

    def _side_extra(self, sst, early):
        """The side stream's extra work of a step, concurrent with the encoder backward: the next step's noise
        and, with an L2 penalty, this step's parameter norms -- the parameters are written by Adam alone, at the
        step's end, behind the epilogue's join with this stream."""
        self._launch_noise(sst, self.idx_next, codecs=('dec',), subset=not early)
        if self.l2 is not None:
            param_norms(self.norms_desc, sst)

    def _build_epilogue(self):
        """The epilogue descriptors over the current engine's scratch and encoder masks."""
        ws = self.engine.ws
        self.epi = L.StepEpilogueDesc(gacc=self.flat.gacc.data_ptr(), grad=self.flat.G.data_ptr(), n=self.flat.numel,
                                      flags=L.FINALIZE_ZERO, n_terms=self.last_terms.numel(),
                                      step=self.step_ctr.data_ptr(), scratch=ws.t_scr.data_ptr(),
                                      n_scratch=ws.t_scr.numel(), terms_dst=self.last_terms.data_ptr(),
                                      idx_src=self.idx_next.data_ptr(), idx_dst=self.idx.data_ptr(),
                                      n_idx=self.n_sub if self.B_u else 0)
        # the next step's encoder Dropout2d masks: drawn by the epilogue (after the encoder backward,
        # which reads this step's), Philox sub id 4 as _launch_noise(sub0=0) would
        ep = self.engine.ep
        if ep is not None and ep.drop_numel > 0:
            self.epi.drop_out = self.engine.ws.fptr(ep.drop_off).value
            self.epi.drop_n = ep.drop_numel
            self.epi.drop_p = ep.drop_rate
            self.epi.drop_seed = self.seed
            self.epi.drop_offset = self.rng_off.data_ptr()
            self.epi.drop_sub = 4
        if self.l2 is not None:
            self.epi.pen_src = self.l2_pen.data_ptr()
            self.epi.pen_dst = self.last_pen.data_ptr()
            if self.distributed:
                # data parallel: into the all-reduced gradient, once on every rank, by the Adam launch (ahead of
                # the SUM it would count `world` times; on one rank alone it would be rounded into that rank's
                # partial gradient, which can be far larger than the sum)
                self.adam.pen_grad = self.pen_grad.data_ptr()
                self.adam.pen_n = self.pen_n
            else:
                self.epi.pen_grad = self.pen_grad.data_ptr()
                self.epi.pen_n = self.pen_n
        self.epi_adam = L.StepEpilogueDesc.from_buffer_copy(self.epi)
        self.epi_adam.step = None                  # Adam's counter: incremented once by the fused launch

    def _wire_handoff(self, probe=True):
        """Flag hand-offs of the current engine (probe: verify the stream pair's hardware queues first)."""
        if self.handoff == 'flags':
            self._configure_handoff(probe)
            if self.fuse_adam:
                # the join with the side stream's last reduction inside the fused epilogue + Adam launch
                self.epi_adam.wait_flag = self.handoff_flags.data_ptr() + 4 * 3
                self.epi_adam.wait_err = self.handoff_flags.data_ptr() + 4 * 4
            # a timed-out hand-off (sticky error word) stops every later parameter update: the gradient of
            # such a step may be incomplete, so no step after it may move the parameters
            self.adam.wait_err = self.handoff_flags.data_ptr() + 4 * 4
            if self.distributed and self.flat.err_slot >= 0:
                # data parallel: the epilogue writes the word into the flat gradient's error slot (inside the
                # all-reduced prefix) and Adam reads the SUM, so one rank's timeout stops every rank's update
                # (and sets every rank's word: all of them raise) -- no rank applies a gradient averaged with
                # an incomplete one
                self.epi.wait_err = self.handoff_flags.data_ptr() + 4 * 4
                self.epi.err_slot = self.flat.err_slot
                self.adam.skip_if = self.flat.G.data_ptr() + 4 * self.flat.err_slot

    def _vo_sources(self):
        """The VO ensemble's (mean, logsigma) fp32 buffers the y_vo draw reads at launch; raises before a
        posterior exists and when the ensemble no longer holds the buffers the step was built on."""
        if self.vo.mean is None:
            raise RuntimeError(NO_POSTERIOR)
        mean, ls = vo_buffers(self.vo)
        if (mean.data_ptr(), ls.data_ptr()) != self._vo_ptrs:
            raise L.NativeError('FusedElboStep: the VO ensemble replaced its mean / logsigma buffers; the step '
                                '(and its captured graphs) reads the old ones: rebuild the step')
        return mean, ls

    def _launch_subset(self, st, idx, sub0=0):
        if not self.B_u:
            return
        if self._subset_ws is None:       # pools up to 16384: one launch, the keys in LDS
            L.check(L.lib().gpi_random_subset(L.ptr(idx), self.n_pool, self.n_sub, self.subset_seed,
                                              L.ptr(self.rng_off), sub0 + 1, st), 'random subset')
        else:                             # any pool (the reference's randperm(N) has no cap)
            L.check(L.lib().gpi_random_subset_ws(L.ptr(idx), self.n_pool, self.n_sub, self.subset_seed,
                                                 L.ptr(self.rng_off), sub0 + 1, L.ptr(self._subset_ws),
                                                 self._subset_ws.numel(), st), 'random subset')

    def _launch_noise(self, st, idx, sub0=0, codecs=('enc', 'dec'), subset=True):
        """Random subset into ``idx`` and the reparametrisation noise into the engine's eps
        buffers.  Philox streams: the step's offset (advanced by Adam at the end of every step)
        and sub ids sub0 + {1, 2, 3}; the noise drawn during step k (for step k+1) therefore
        differs from step k's own, which was drawn during step k-1 or by the prologue (sub0 = 100).
        With the VO term active also its targets y_vo ~ N(VO.mean, VO.var) (sub id sub0 + 6), read from the
        ensemble's buffers when the launch runs: a replay draws from the posterior the last update wrote.
        All of it in ONE launch (gpi_draws: the same draws as the separate entry points, bit for bit)
        unless the pool needs the multi-launch subset form or GPI_ONE_DRAW=0."""
        lib = L.lib()
        if self._one_draw and (not subset or not self.B_u or self._subset_ws is None):
            items = []
            e = self.engine
            if e.has_dropout and codecs:
                for k, (c, prog) in enumerate((('enc', e.ep), ('dec', e.dp))):
                    if c in codecs and prog is not None and prog.drop_numel:
                        items.append(L.DrawItem(kind=L.DRAW_DROPOUT, p=prog.drop_rate, out=e.ws.fptr(prog.drop_off).value,
                                                n=prog.drop_numel, sub=sub0 + 4 + k, seed=self.seed))
            if subset and self.B_u:     # (the subset's key: the seed every rank shares)
                items.append(L.DrawItem(kind=L.DRAW_SUBSET, out=idx.data_ptr(), n=self.n_pool, k=self.n_sub,
                                        sub=sub0 + 1, seed=self.subset_seed))
            ez = e.eps_z()
            items.append(L.DrawItem(kind=L.DRAW_RANDN, out=ez.data_ptr(), n=ez.numel(), sub=sub0 + 2, seed=self.seed))
            if e.N_ex:
                ex = e.eps_x()
                items.append(L.DrawItem(kind=L.DRAW_RANDN, out=ex.data_ptr(), n=ex.numel(), sub=sub0 + 3,
                                        seed=self.seed))
            if e.N_vo and not e.vo_holdoff:
                yv = e.y_vo()
                mean, ls = self._vo_sources()
                items.append(L.DrawItem(kind=L.DRAW_GAUSS, out=yv.data_ptr(), n=yv.numel(), sub=sub0 + VO_Y_SUB,
                                        seed=self.seed, mean=mean.data_ptr(), logsigma=ls.data_ptr()))
            arr = (L.DrawItem * len(items))(*items)
            L.check(lib.gpi_draws(arr, len(items), L.ptr(self.rng_off), st), 'step draws')
            return
        if self.engine.has_dropout and codecs:   # Dropout2d channel scales (sub ids sub0 + 4 enc, + 5 dec)
            self.engine.draw_dropout(st, self.seed, L.ptr(self.rng_off), sub0 + 4, codecs=codecs)
        if subset:
            self._launch_subset(st, idx, sub0)
        ez = self.engine.eps_z()
        L.check(lib.gpi_randn(L.ptr(ez), ez.numel(), self.seed, L.ptr(self.rng_off), sub0 + 2, st), 'randn z')
        if self.engine.N_ex:
            ex = self.engine.eps_x()
            L.check(lib.gpi_randn(L.ptr(ex), ex.numel(), self.seed, L.ptr(self.rng_off), sub0 + 3, st), 'randn x')
        if self.engine.N_vo and not self.engine.vo_holdoff:
            mean, ls = self._vo_sources()
            gvo.gauss_sample(self.engine.y_vo(), mean, ls, seed=self.seed, offset=self.rng_off, sub=sub0 + VO_Y_SUB,
                             stream=st)

    def forward_backward(self, stream=None):
        """One step without the parameter update (gradient in flat.G and the ELBO terms delivered;
        update() then applies Adam).  Every forward_backward() must be followed by update() before the
        next one: the cross-stream flags count one signal per step, and the step counter that their waits
        compare against advances only in the update (an unpaired pass would leave the flags ahead and every
        later wait would pass at once)."""
        if self._fb_pending:
            raise RuntimeError('FusedElboStep.forward_backward() called twice without update() in between')
        self._forward_backward(stream, epilogue=True)
        self.engine.rejoin()
        self._fb_pending = True

    def _forward_backward(self, stream=None, epilogue=True):
        """One step without the parameter update.  The step's noise and subset were drawn by the
        previous step (off the critical path); the next step's are drawn on the side stream once
        the head backward has consumed this step's; the epilogue (gradient finalisation, scratch
        reset, subset hand-over) is one launch."""
        st = stream if stream is not None else L.stream_handle()
        # subset_early: the next step's subset (it writes only idx_next) ahead of the ROM on the side stream
        early = self.subset_early and bool(self.engine.roms)
        self.engine.side_pre = (lambda sst: self._launch_subset(sst, self.idx_next)) if early else None
        self.engine.forward(st, compute_value=False, zero_gacc=False, zero_scratch=False, running='defer')
        # next step's subset / noise / decoder masks concurrently with the encoder backward; the
        # encoder's masks by the epilogue below (the encoder backward reads this step's)
        # the fused epilogue + Adam launch (update(fused=True)) waits for the side stream itself; every
        # other continuation needs the main stream to wait here
        self.engine.backward(st, side_extra=lambda sst: self._side_extra(sst, early),
                             main_wait=epilogue or not self.fuse_adam)
        if epilogue:                  # (else: launched by update(fused=True), with Adam)
            L.check(L.lib().gpi_step_epilogue(C.byref(self.epi), st), 'step epilogue')

    def allreduce(self):
        if self.distributed:
            allreduce_shared(self.flat, self.pg)

    def sync_lr(self):
        """Copy a scheduler-changed learning rate (optimizer.param_groups[0]['lr']) to the device."""
        lr = float(self.optimizer.param_groups[0]['lr'])
        if lr != self._lr_host:
            self.lr.fill_(lr)
            self._lr_host = lr

    def update(self, stream=None, fused=False):
        """Adam (+ RNG offset advance).  fused: the step epilogue and Adam in one launch -- after
        _forward_backward(epilogue=False), single-process steps only."""
        st = stream if stream is not None else L.stream_handle()
        self._fb_pending = False
        if fused:
            L.check(L.lib().gpi_step_epilogue_adam(C.byref(self.epi_adam), C.byref(self.adam),
                                                   L.ptr(self.done_ctr), st), 'step epilogue + adam')
        else:
            L.check(L.lib().gpi_adam(C.byref(self.adam), st), 'adam (+ rng offset advance)')

    def _mark_optimizer_step(self):
        """Tell torch LR schedulers that an optimizer step happened (their hook wraps
        optimizer.step() to set this flag; calling the wrapped no-op through torch's profiling
        hooks costs ~0.2 ms of host time per step, as much as a third of the step)."""
        self.optimizer._opt_called = True

    def step_eager(self):
        self._check_label_mask()
        self._check_stream_pair()
        fused = self.fuse_adam
        self._forward_backward(epilogue=not fused)
        self.allreduce()
        self.update(fused=fused)
        self.engine.rejoin()
        self._mark_optimizer_step()

    def check_handoff(self):
        """Raise if a side-stream flag wait timed out (host sync).  The step that timed out and every step
        after it have left the parameters and Adam moments untouched (the error word is sticky)."""
        if int(self.handoff_flags[4].item()) != 0:
            raise RuntimeError('FusedElboStep: a cross-stream flag wait timed out (gpi_stream_wait); '
                               'parameter updates were skipped from that step on')

    def _poll_error(self):
        """Raise if the last posted copy of the error word (see _post_error_copy) shows a timed-out wait;
        never blocks (an unfinished copy is read at a later call)."""
        ev = self._err_ev
        if ev is not None and ev.query():
            self._err_ev = None
            if int(self._err_host[0]) != 0:
                raise RuntimeError('FusedElboStep: a cross-stream flag wait timed out (gpi_stream_wait); '
                                   'parameter updates were skipped from that step on')

    def _post_error_copy(self):
        if self._err_host is None or self.handoff != 'flags' or self._err_ev is not None:
            return
        self._err_host.copy_(self.handoff_flags[4:5], non_blocking=True)
        self._err_ev = torch.cuda.Event()
        self._err_ev.record()

    # ------------------------------------------------------------------
    def _mutable_state(self):
        """Every device buffer a step writes: parameters, Adam moments and counter, Philox offset,
        subsets, accumulators, gradient, the workspace (incl. the pre-drawn noise) and the term /
        statistics scratch."""
        ws = self.engine.ws
        l2 = [] if self.l2 is None else [self.pen_grad, self.l2_norms, self.l2_pen, self.last_pen, self.l2_done]
        return [self.flat.P, self.m, self.v, self.step_ctr, self.rng_off, self.idx, self.idx_next, self.done_ctr,
                self.handoff_flags, self.side_done,
                self.flat.gacc, self.flat.G, ws.t_ws, ws.t_scr, ws.t_parts, ws.t_flag, self.last_terms] + l2 + \
            self.engine.running.buffers

    def capture(self, unroll=1):
        """Capture the step into HIP graph(s); the all-reduce stays outside the graph.
        The two warm-up steps run on snapshots: capture() leaves parameters, optimizer state,
        step counter, random stream and the pre-drawn subset / noise exactly as it found them, so
        the first replayed step is the step an eager loop would take next.
        unroll > 1 ('streams' mode): also capture `unroll` consecutive steps as one pair of graphs, which
        run(n) replays (one graph-launch boundary per `unroll` steps; every step still reads its counters,
        subset, noise and learning rate from device memory, so the steps are the ones step() would take --
        a learning-rate change reaches the device at the next replay)."""
        self.unroll = 1
        self.g_fb_k = self.g_side_k = None
        if self.sync_bn and self.bn_exchange != 'peer' and dist.get_backend(self.pg) != dist.Backend.NCCL:
            raise RuntimeError('FusedElboStep.capture: SyncBN over a host-side backend (gloo) runs eagerly only '
                               "(bn_exchange='peer' captures with any backend)")
        torch.cuda.synchronize()
        saved = [t.clone() for t in self._mutable_state()]
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):          # warm up allocator / kernels on the side stream
                self.step_eager()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        self.check_handoff()            # (the restore below would erase a warm-up step's timeout)
        for t, v in zip(self._mutable_state(), saved):
            t.copy_(v)
        del saved
        torch.cuda.synchronize()
        self.g_fb = torch.cuda.CUDAGraph()
        self.g_up = None
        self.g_side = None
        self.segs = None
        self.split_graph = self.distributed and not (self.graph_allreduce and
                                                      dist.get_backend(self.pg) == dist.Backend.NCCL)
        if not self.split_graph and self.graph_mode == 'segments':
            self._capture_segments()
        elif not self.split_graph and self.graph_mode == 'streams':
            self._capture_streams()
            if unroll > 1:
                self.g_fb_k, self.g_side_k = self._capture_streams(unroll)
                self.unroll = int(unroll)
        elif self.split_graph:
            with torch.cuda.graph(self.g_fb):
                self.forward_backward()
                self.engine.rejoin()
            self.g_up = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.g_up):
                self.update()
        else:
            fused = self.fuse_adam
            with torch.cuda.graph(self.g_fb):
                self._forward_backward(epilogue=not fused)
                self.allreduce()        # RCCL: captured as a graph node
                self.update(fused=fused)
                self.engine.rejoin()
        self.graph = True

    def _queues_separate(self):
        """True iff a kernel on the current stream runs while a kernel of the side stream spins
        (gpi_queue_probe): the two are on different hardware queues.  HIP maps streams to its
        GPU_MAX_HW_QUEUES queues round-robin, so in a process with many streams two can share one, and
        a flag wait ahead of its signal on a shared queue blocks it (tools/queue_stress.py: 3 of 18
        steps timed out with 6 step objects in 'streams' mode, none in 'single', whose graph
        branches the runtime places itself)."""
        e = self.engine
        pr = torch.zeros(2, dtype=torch.int32, device=self.flat.P.device)
        # up to four side-stream candidates (HIP deals new streams round-robin over its queues, so one of
        # four consecutive ones sits on another queue than the current stream); a replaced candidate is
        # dropped before any work or capture used it
        for attempt in range(4):
            side = e._side_stream()
            pr.zero_()
            torch.cuda.synchronize()
            L.check(L.lib().gpi_queue_probe(L.ptr(pr), L.ptr(pr[1:]), C.c_void_p(side.cuda_stream)), 'queue probe')
            L.check(L.lib().gpi_stream_signal(L.ptr(pr), L.ptr(self.step_ctr), L.stream_handle()),
                    'queue probe signal')
            torch.cuda.synchronize()
            self._probed_stream = torch.cuda.current_stream()
            if int(pr[1].item()) == 1:
                return True
            if getattr(self, 'graph', None) is not None:
                return False        # the captured graphs hold this side stream
            e._side = None          # next candidate
        return False

    def _configure_handoff(self, probe=True):
        """Flag hand-offs between the streams; graph mode 'streams' (no event between the streams at all)
        only on a verified pair of hardware queues, else 'single' (one graph whose event fork / join at
        its ends the runtime orders)."""
        if probe and self.graph_mode == 'streams' and not self._queues_separate():
            self.graph_mode = 'single'
        self.engine.set_flag_handoff(self.handoff_flags[:4], self.step_ctr, self.handoff_flags[4:5],
                                     side_done=self.side_done if self.graph_mode == 'streams' else None)

    def _check_stream_pair(self):
        """'streams' mode, before a step: the probe was made against another current stream -- probe this
        one; on a shared queue fall back to 'single' (and capture again if the step was captured)."""
        if self.graph_mode != 'streams' or torch.cuda.current_stream() == self._probed_stream:
            return
        if self._queues_separate():
            return
        self.graph_mode = 'single'
        self._configure_handoff()
        if self.graph is not None:
            self.capture()          # ('single': no unrolled graphs; run() replays single steps)

    def _capture_streams(self, steps=1):
        """The step as TWO graphs, one per stream, captured at once: the main stream's (encoder, head,
        decoder, their backward, the epilogue + Adam) and the side stream's (ROM, the variational samples'
        head backward, the slab reductions, the next step's noise), ordered only by the device counters
        of the flag hand-offs and the side stream's step gate -- no graph edge between the streams.
        steps > 1: that many consecutive steps in the pair, returned as (main, side) graphs."""
        fused = self.fuse_adam
        side = self.engine._side_stream()
        cap = torch.cuda.Stream()
        cap.wait_stream(torch.cuda.current_stream())
        side.wait_stream(torch.cuda.current_stream())
        g_fb = self.g_fb if steps == 1 else torch.cuda.CUDAGraph()
        g_side = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            g_side.capture_begin(capture_error_mode='relaxed')
        try:
            with torch.cuda.stream(cap):
                g_fb.capture_begin(capture_error_mode='relaxed')
                try:
                    for _ in range(steps):
                        self._forward_backward(epilogue=not fused)
                        self.allreduce()        # RCCL: captured as a graph node
                        self.update(fused=fused)
                finally:
                    g_fb.capture_end()
        finally:
            with torch.cuda.stream(side):
                g_side.capture_end()
        torch.cuda.current_stream().wait_stream(cap)
        if steps == 1:
            self.g_side = g_side
        return g_fb, g_side

    def _capture_segments(self):
        """The segment joiner: the step as single-stream graphs, one per stretch of the schedule table
        (gpi.schedule.segments), replayed with events for the table's edges (_replay_segments).  A HIP graph whose
        nodes span two streams costs the host ~4-8 us per node to launch (tools/graph_launch_probe.py:
        64 nodes 211-245 us on two streams vs 50-58 us on one); with the step's ~70 nodes in one
        two-stream graph the host walk (~0.59 ms) paced the GPU and the side stream's kernels were
        submitted late, so the step waited at the join for them."""
        e = self.engine
        e.handoff = None                     # the segments are joined by events between the graphs
        self.epi_adam.wait_flag = None
        self.epi_adam.wait_err = None
        early = self.subset_early and bool(e.roms)
        e.side_pre = (lambda sst: self._launch_subset(sst, self.idx_next)) if early else None
        extra = {'forward_a': dict(zero_gacc=False, zero_scratch=False),
                 'backward_side_a': dict(side_extra=lambda sst: self._side_extra(sst, early))}

        def tail(st):
            fused = self.fuse_adam
            if not fused:
                L.check(L.lib().gpi_step_epilogue(C.byref(self.epi), st), 'step epilogue')
            self.allreduce()                     # RCCL: captured as a graph node
            self.update(st, fused=fused)

        def cap(seg):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                st = L.stream_handle()
                for s in seg.rows:
                    if s.piece is None:          # the main stream's continuation behind the side stream's end
                        tail(st)
                    else:
                        getattr(e, s.piece)(st, **dict(s.args, **extra.get(s.piece, {})))
            return g

        # the table of the value not read after the forward and the BN running statistics deferred to the side
        # stream; it has no rom_at / rom_first arm in this mode (ElboEngine.schedule)
        self.segs = [(seg, cap(seg)) for seg in segments(e.schedule(False, 'defer', segments=True))]
        self._seg_ev = {k: torch.cuda.Event() for k in (E_ROM, E_DEC, E_ENC, E_SIDE)}
        self._seg_side = e._side_stream()

    def _replay_segments(self):
        """The segment joiner's replay: the table's edges as events between the graphs."""
        ev = self._seg_ev
        streams = {MAIN: torch.cuda.current_stream(), SIDE: self._seg_side}
        for seg, g in self.segs:
            st = streams[seg.stream]
            with torch.cuda.stream(st):
                if seg.wait is not None:
                    st.wait_event(ev[seg.wait])
                g.replay()
            if seg.signal is not None:
                ev[seg.signal].record(st)

    def step(self):
        """One training step (graph replay once captured).  A timed-out cross-stream wait raises at a
        later step() (its error word is copied back every GPI_ERR_CHECK_EVERY steps, no host sync)."""
        self._poll_error()
        self._step()
        self._n_steps += 1
        if self._err_every > 0 and self._n_steps % self._err_every == 0:
            self._post_error_copy()

    def _step(self):
        self._check_label_mask()
        self.sync_lr()
        if self.graph is None:
            return self.step_eager()
        if self.segs is not None:
            self._replay_segments()
            self._mark_optimizer_step()
            return
        if self.g_side is not None:
            self._check_stream_pair()
        if self.g_side is not None:
            # (the side graph launched first instead: 0.5772-0.5774 vs 0.5767-0.5769 ms, r04k)
            self.g_fb.replay()
            with torch.cuda.stream(self.engine._side):
                self.g_side.replay()
            self._mark_optimizer_step()
            return
        self.g_fb.replay()
        if self.split_graph:
            self.allreduce()
            self.g_up.replay()
        self._mark_optimizer_step()

    def run(self, n):
        """n steps: with capture(unroll=k), n // k replays of the k-step graphs, then single steps."""
        n = int(n)
        self._poll_error()
        self._check_label_mask()
        if self.graph is not None and self.unroll > 1 and self.g_fb_k is not None:
            self.sync_lr()
            self._check_stream_pair()
            if self.graph_mode == 'streams' and self.g_fb_k is not None:
                for _ in range(n // self.unroll):
                    self.g_fb_k.replay()
                    with torch.cuda.stream(self.engine._side):
                        self.g_side_k.replay()
                    self._mark_optimizer_step()
                n %= self.unroll
        for _ in range(n):
            self._step()
        self._post_error_copy()

    def elbo(self):
        """ELBO value of the last completed step (0-d tensor), less the step's L2 penalty (data parallel: on rank 0
        alone, so the ranks' values still sum to the global objective)."""
        val = self.engine.elbo_value(self.last_terms)
        if self.l2 is not None and self.rank == 0:
            val = (val.double() - self.last_pen[1]).to(torch.float32)
        return val

    def terms(self):
        """The individual ELBO terms of the last completed step (ElboEngine.terms; host sync); with an L2 penalty
        also 'elbo_l2_penalty', the sum of the parameter norms (the reference's scalar tag)."""
        out = self.engine.terms(self.last_terms)
        if self.l2 is not None:
            out['elbo_l2_penalty'] = float(self.last_pen[0])
        return out

    # ------------------------------------------------------------------ virtual observables
    def _require_vo(self, what):
        if not self.N_vo:
            raise L.NativeError('FusedElboStep.%s: the step was built without X_vo' % what)
        if self._fb_pending:
            raise RuntimeError('FusedElboStep.%s between forward_backward() and update(): the pending update '
                               'still reads this step\'s gradient and noise' % what)

    @torch.no_grad()
    def update_virtual_observables(self, N_monte_carlo, step, eps=None, Resample=True):
        """The loop's VO update (training.py:407-409) between two steps: model.update_virtual_observables,
        which writes the ensemble's posterior buffers in place, then a redraw of the pending target y_vo
        from the new posterior (the next step's was drawn during the previous step's backward from the old
        one; the reference draws y at elbo() time, after the update).  The redraw runs eagerly at the
        current Philox offset, sub id VO_REDRAW_SUB.  Ordered by device synchronisation after the previous
        step's work on both streams and before the next replay (a host-bound ~1 ms call once per update
        interval); captured graphs stay valid: they read the ensemble's buffers at launch."""
        self._require_vo('update_virtual_observables')
        torch.cuda.synchronize()
        self.model.update_virtual_observables(N_monte_carlo, step=step, eps=eps, Resample=Resample)
        mean, ls = self._vo_sources()
        if not self.engine.vo_holdoff:
            gvo.gauss_sample(self.engine.y_vo(), mean, ls, seed=self.seed, offset=self.rng_off, sub=VO_REDRAW_SUB)
        torch.cuda.synchronize()

    def set_vo_holdoff(self, flag):
        """training.py:411's ``gn < N_vo_holdoff`` switch: rebuild the engine for the other variant of the VO
        term on the same flat parameters and draw that engine's pending noise (masks, eps_z, eps_X, y_vo:
        sub ids VO_SWITCH_SUB0 + {2 .. 6} at the current Philox offset; the pending subset stays).
        Parameters, Adam moments, step counter, Philox offset, learning rate, scheduler handle and BN
        running buffers are untouched.  Captured graphs are dropped: step() runs eagerly until the next
        capture().  elbo() / terms() of the last step before the switch are to be read before it."""
        self._require_vo('set_vo_holdoff')
        flag = bool(flag)
        if flag == self.engine.vo_holdoff:
            return
        if not flag:
            self._vo_sources()              # (no posterior yet: raise before anything changes)
        torch.cuda.synchronize()
        old = self.engine
        new = self._new_engine(flag)
        # the stream pair (probed hardware queues) and its events go with the step, not the engine
        for k in ('_side', '_ev'):
            if hasattr(old, k):
                setattr(new, k, getattr(old, k))
        new.ws.t_flag.copy_(old.ws.t_flag)  # (the ROM's sticky conductivity flag: check_flag)
        if self.sync_bn:
            self._set_sync_bn(new)
        self._bind(new)
        self.engine = new
        self._build_epilogue()
        self._wire_handoff(probe=False)
        self.graph = None
        self.g_fb = self.g_up = self.g_side = self.segs = None
        self.g_fb_k = self.g_side_k = None
        self.unroll = 1
        self._launch_noise(L.stream_handle(), self.idx, sub0=VO_SWITCH_SUB0, subset=False)
        torch.cuda.synchronize()
