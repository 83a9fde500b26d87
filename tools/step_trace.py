"""Launch trace of the training step's host side: what is launched, on which stream, in which order, behind which
event, with which descriptor contents -- as text that does not depend on addresses, so that two Python trees over
the same native library can be compared byte for byte (a refactor of gpi/engine.py, gpi/train.py must leave it alone).

    python tools/step_trace.py [--tree DIR] [--out FILE] [--arms a,b,...]      # driver: every arm, one child each
    python tools/step_trace.py [--tree DIR] --arm NAME                         # one arm, trace on stdout
    python tools/step_trace.py --compact FILE                                  # a trace with structure bodies hashed

--tree: the repository tree whose gpi package and tests/ helpers are used (default: this one); its
gpi/libgpi_hip.so must exist.  The tool hooks only what every tree has: the loaded library object (gpi._lib._LIB
becomes a recording proxy) and torch (Event.record, Stream.wait_event / wait_stream, CUDAGraph.capture_begin /
capture_end / replay).  Per native call it writes the entry point, the stream (named main, side, other<k> by
first appearance), every scalar argument, and of every ctypes structure argument (arrays element by element) the
fields that are not addresses; an address prints as 0, * or, inside a registered buffer, name+offset (the hand-off
flag words).  Events and graphs are numbered by first appearance.

Each arm runs in a fresh child process under its own time limit, one after another; the driver stops at the first
failure.  A 'streams' arm that fell back to 'single' (the two streams share a hardware queue) says so in its trace.
"""
import argparse
import ctypes as C
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ARM_TIMEOUT = 240

FUSED = 'GPI_GRAPH_MODE GPI_HANDOFF GPI_ROM_EARLY GPI_ROM_AT GPI_ENC_REDUCE GPI_FUSE_OUT'.split()
# name -> (environment, body, body arguments)
ARMS = {}
for mode in ('streams', 'single', 'segments'):
    for hand in ('flags', 'events'):
        ARMS['fused_%s_%s' % (mode, hand)] = ({'GPI_GRAPH_MODE': mode, 'GPI_HANDOFF': hand}, 'fused', {})
ARMS.update({
    'fused_rom_early': ({'GPI_ROM_EARLY': '1'}, 'fused', {}),
    'fused_rom_at_backward': ({'GPI_ROM_AT': 'backward'}, 'fused', {}),
    'fused_enc_reduce_main': ({'GPI_ENC_REDUCE': 'main'}, 'fused', {}),
    'fused_fuse_out_0': ({'GPI_FUSE_OUT': '0'}, 'fused', {}),
    'fused_rom_first': ({}, 'fused', {'rom_first': True}),
    'fused_subset_early': ({}, 'fused', {'subset_early': True}),
    'vo': ({}, 'fused', {'fixture': 'vo'}),
    'vo_holdoff': ({}, 'fused', {'fixture': 'vo', 'holdoff': True}),
    'vo_lockx': ({}, 'fused', {'fixture': 'vo_lockx'}),
    'gpmlp': ({}, 'fused', {'fixture': 'gpmlp'}),
    'nonarm_module_path': ({}, 'nonarm', {}),
    'module_path': ({}, 'module_path', {}),
    'prediction_ensemble': ({}, 'prediction_ensemble', {}),
    'codec_engines': ({}, 'codec_engines', {}),
    'eval_engines': ({}, 'eval_engines', {}),
})


# ---------------------------------------------------------------------------------------------- recording
class Trace(object):
    def __init__(self):
        self.lines, self.streams, self.events, self.graphs, self.regions = [], {}, {}, {}, []

    def write(self, text):
        self.lines.append(text)

    def stream(self, handle):
        h = int(handle or 0)
        if h not in self.streams:
            k = len(self.streams)
            self.streams[h] = ('main', 'side')[k] if k < 2 else 'other%d' % k
        return self.streams[h]

    def numbered(self, table, obj, prefix):
        return prefix + str(table.setdefault(id(obj), (len(table), obj))[0])      # (kept alive: ids stay unique)

    def addr(self, v):
        v = int(v or 0)
        if not v:
            return '0'
        for name, base, size in self.regions:
            if base <= v < base + size:
                return '%s+%d' % (name, v - base)
        return '*'

    def struct(self, s):
        out = []
        for name, typ in s._fields_:
            if name.startswith('_'):
                continue
            v = getattr(s, name)
            if typ is C.c_void_p:
                out.append('%s=%s' % (name, self.addr(v)))
            elif issubclass(typ, C.Structure):
                out.append('%s=%s' % (name, self.struct(v)))
            elif issubclass(typ, C.Array):
                items = [self.addr(x) for x in v] if typ._type_ is C.c_void_p else [repr(x) for x in v]
                out.append('%s=[%s]' % (name, ','.join(items)))
            else:
                out.append('%s=%r' % (name, v))
        return '%s(%s)' % (type(s).__name__, ' '.join(out))

    def native(self, name, argtypes, args):
        parts = []
        has_stream = bool(argtypes) and argtypes[-1] is C.c_void_p and not name.startswith(('gpi_peer', 'gpi_conv_shape'))
        for i, a in enumerate(args):
            if has_stream and i == len(args) - 1:
                parts.insert(0, 'stream=' + self.stream(getattr(a, 'value', a)))
            elif isinstance(a, C.Structure):
                parts.append(self.struct(a))
            elif hasattr(a, '_obj'):                                                 # byref(struct), byref(output)
                parts.append(self.struct(a._obj) if isinstance(a._obj, C.Structure) else '*')
            elif isinstance(a, C.Array):
                parts.append('[%s]' % ' '.join(self.struct(x) if isinstance(x, C.Structure) else repr(x) for x in a))
            elif isinstance(a, C._Pointer):                                          # element pointer + count
                parts.append('[%s]' % ' '.join(self.struct(a[j]) for j in range(int(args[i + 1]))))
            elif isinstance(a, C.c_void_p) or (i < len(argtypes) and argtypes[i] is C.c_void_p):
                parts.append(self.addr(getattr(a, 'value', a)))
            else:
                parts.append(repr(getattr(a, 'value', a)))
        self.write('%s %s' % (name, ' '.join(parts)))


class LibProxy(object):
    def __init__(self, lib, trace):
        self.__dict__['_lib'], self.__dict__['_trace'] = lib, trace

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*args):
            self._trace.native(name, fn.argtypes or [], args)
            return fn(*args)
        return call


def install(trace):
    import torch
    from gpi import _lib as L
    L._LIB = LibProxy(L.lib(), trace)
    cur = lambda: trace.stream(torch.cuda.current_stream().cuda_stream)
    sname = lambda s: trace.stream(s.cuda_stream) if s is not None else cur()

    def wrap(cls, name, describe):
        orig = getattr(cls, name)

        def f(self, *a, **k):
            trace.write(describe(self, *a, **k))
            return orig(self, *a, **k)
        setattr(cls, name, f)

    ev = lambda e: trace.numbered(trace.events, e, 'e')
    gr = lambda g: trace.numbered(trace.graphs, g, 'g')
    wrap(torch.cuda.Event, 'record', lambda e, stream=None: 'event.record %s stream=%s' % (ev(e), sname(stream)))
    wrap(torch.cuda.Stream, 'wait_event', lambda s, e: 'stream.wait_event %s stream=%s' % (ev(e), sname(s)))
    wrap(torch.cuda.Stream, 'wait_stream', lambda s, o: 'stream.wait_stream stream=%s on=%s' % (sname(s), sname(o)))
    wrap(torch.cuda.CUDAGraph, 'capture_begin', lambda g, *a, **k: 'graph.capture_begin %s stream=%s' % (gr(g), cur()))
    wrap(torch.cuda.CUDAGraph, 'capture_end', lambda g: 'graph.capture_end %s stream=%s' % (gr(g), cur()))
    wrap(torch.cuda.CUDAGraph, 'replay', lambda g: 'graph.replay %s stream=%s' % (gr(g), cur()))


# ---------------------------------------------------------------------------------------------- arms
def fused(trace, fixture='elbo', holdoff=False, rom_first=False, subset_early=False):
    """One step_eager(), capture() and two step() of a FusedElboStep built as the tests build it."""
    import torch
    from gpi.train import FusedElboStep
    if fixture == 'elbo':
        from test_gpu_parity import load, cuda, build_golden_model
        d = load('elbo_c32.npz')
        model, bs = build_golden_model(d)
        step = FusedElboStep(model, cuda(d['Xu']), bs, cuda(d['Xs']), cuda(d['Y']), cuda(d['F']), lr=1e-3, seed=3)
    elif fixture == 'gpmlp':
        import test_gpu_gp_mlp_elbo as T
        d = T.load_case(T.CASES[0])
        model, bs = T.mlp_model(d)
        step = T._step(d, model, bs)
    else:
        import test_gpu_fused_vo as T
        d, model, ens, bs = T.vo_model(fixture == 'vo_lockx')
        step = T.make_step(d, model, bs, vo_holdoff=holdoff)
    trace.regions.append(('flags', step.handoff_flags.data_ptr(), 4 * step.handoff_flags.numel()))
    want = os.environ.get('GPI_GRAPH_MODE', 'streams')
    trace.write('# built: graph_mode=%s handoff=%s%s' % (step.graph_mode, step.handoff, '' if step.graph_mode == want
                else ' (fell back from %s)' % want))
    step.engine.rom_first = rom_first
    step.subset_early = subset_early
    trace.write('# step_eager')
    step.step_eager()
    trace.write('# capture')
    step.capture()
    trace.write('# captured: graph_mode=%s handoff=%s engine.handoff is None: %s' % (
        step.graph_mode, step.handoff, step.engine.handoff is None))
    for _ in range(2):
        trace.write('# step')
        step.step()
    torch.cuda.synchronize()
    step.check_handoff()
    step.engine.check_flag()


def module_path(trace):
    """GenerativeModel.elbo + backward: ElboEngine.forward(compute_value=True) and backward()."""
    import torch
    from test_gpu_parity import load, cuda, build_golden_model
    d = load('elbo_c32.npz')
    model, bs = build_golden_model(d)
    eps = (torch.cat([cuda(d['eps_enc']), cuda(d['eps_qz'])]), cuda(d['eps_qX']))
    trace.write('# elbo')
    elbo = model.elbo(step=0, armortized_bs=bs, eps=eps)
    trace.write('# backward')
    (-elbo).backward()
    torch.cuda.synchronize()


def nonarm(trace):
    """The non-armortized fixture through the module path, built as test_elbo_nonarmortized_matches_reference does."""
    import torch
    from test_gpu_parity import load, cuda, _DS
    from bottleneck.Decoder import CNNDecoder
    from bottleneck.components import EffectivePropertyMap, ReducedOrderModelOperator
    from bottleneck.ROM import ROM
    from bottleneck.generative import GenerativeModel
    from physics.grid import StructuredGrid
    d = load('elbo_nonarm_c32.npz')
    n, nc, dz, Nu, Ns = [int(v) for v in d['cfg']]
    dec = CNNDecoder(n, dz, (8, 8), 1, 4, [1, 1], False, 4, drop_rate=0.)
    g = ReducedOrderModelOperator(ROM(StructuredGrid(nc), n // nc), torch.tensor(d['W']), dtype=torch.float32,
                                  device='cuda')
    gp = EffectivePropertyMap(dz, 2 * nc * nc, dtype=torch.float32, device='cuda')
    model = GenerativeModel(f=dec.cuda(), g=g, gp=gp, dtype=torch.float32, device=torch.device('cuda'))
    model.register_datasets({'supervised': _DS(X=cuda(d['Xs']), Y=cuda(d['Y']), F_ROM_BC=cuda(d['F'])),
                             'unsupervised': _DS(X=cuda(d['Xu']))}, None,
                            create_unsupervised_variational_approximation=True)
    model.load_state_dict({k[6:]: torch.tensor(v) for k, v in d.items() if k.startswith('state.')})
    model.cuda()
    eps = (torch.cat([cuda(d['eps_u']), cuda(d['eps_qz'])]), cuda(d['eps_qX']))
    trace.write('# elbo')
    elbo = model.elbo(step=0, eps=eps)
    trace.write('# backward')
    (-elbo).backward()
    torch.cuda.synchronize()


def prediction_ensemble(trace):
    """One PredictionEnsembleEngine.update() on pe_analysis_c32.npz (through PredictionEnsemble.update)."""
    import torch
    import test_gpu_predictive as T
    from bottleneck.components import PredictionEnsemble
    from lamp.optimization import LearningScheduleWrapper
    d = T.load('pe_analysis_c32.npz')
    model, ds = T.build(d)
    pe = PredictionEnsemble(model, ds, LearningScheduleWrapper.Dummy(), lr=1e-2, writer=T._Writer())
    trace.write('# update')
    pe.update(numIter=1, record=True, step=0, eps=[T.cuda(d['pe_eps'][0])])
    torch.cuda.synchronize()


def codec_engines(trace):
    """One forward and backward of EncoderEngine / DecoderEngine (the modules' native autograd path)."""
    import torch
    from test_gpu_parity import _codec, cuda
    d, enc, dec = _codec('c32')
    trace.write('# encoder')
    mu, ls = enc(cuda(d['X']))
    (torch.sum(mu * cuda(d['enc_wm'])) + torch.sum(ls * cuda(d['enc_ws']))).backward()
    trace.write('# decoder')
    Z = cuda(d['Z']).requires_grad_(True)
    mx, lsx = dec(Z)
    (torch.sum(mx * cuda(d['dec_vm'])) + torch.sum(lsx * cuda(d['dec_vs']))).backward()
    torch.cuda.synchronize()


def eval_engines(trace):
    """One forward of EvalEncoderEngine / EvalDecoderEngine (the modules in .eval())."""
    import torch
    from test_gpu_parity import _codec, cuda
    d, enc, dec = _codec('c32')
    enc.eval()
    dec.eval()
    with torch.no_grad():
        trace.write('# encoder eval')
        enc(cuda(d['X']))
        trace.write('# decoder eval')
        dec(cuda(d['Z']))
    torch.cuda.synchronize()


def run_arm(name, tree):
    pkg = os.path.join(tree, 'generative-physics-informed-pde_amd')
    for p in (os.path.join(tree, 'tests'), pkg, tree):
        sys.path.insert(0, p)
    env, body, kw = ARMS[name]
    import torch
    torch.manual_seed(0)              # module initialisation and host-drawn Philox seeds (gpi.predictive.host_seed)
    trace = Trace()
    install(trace)
    trace.write('== arm %s %s' % (name, ' '.join('%s=%s' % (k, os.environ[k]) for k in FUSED if k in os.environ)))
    try:
        globals()[body](trace, **kw)
    finally:
        sys.stdout.write('\n'.join(trace.lines) + '\n')
        sys.stdout.flush()


def compact(text):
    """A trace with every structure's field list replaced by its sha1 (12 hex digits): the form kept under
    profiles/ (the full text of 21 arms is over a megabyte); equal full traces give equal compact ones."""
    import hashlib
    import re
    head = re.compile(r'[A-Za-z]\w*\(')
    out = []
    for line in text.splitlines():
        if line.startswith(('#', '==')):
            out.append(line)
            continue
        res, i = [], 0
        while True:
            m = head.search(line, i)
            if not m:
                res.append(line[i:])
                break
            j, depth = m.end(), 1
            while depth:
                depth += {'(': 1, ')': -1}.get(line[j], 0)
                j += 1
            res.append(line[i:m.end() - 1] + '#' + hashlib.sha1(line[m.end():j - 1].encode()).hexdigest()[:12])
            i = j
        out.append(''.join(res))
    return '\n'.join(out) + '\n'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--compact', metavar='FILE', help='print the compact form of a trace file')
    ap.add_argument('--tree', default=os.path.dirname(HERE))
    ap.add_argument('--arm')
    ap.add_argument('--arms', default=','.join(ARMS))
    ap.add_argument('--out')
    a = ap.parse_args()
    tree = os.path.abspath(a.tree)
    if a.compact:
        return sys.stdout.write(compact(open(a.compact).read())) and 0
    if a.arm:
        return run_arm(a.arm, tree)
    out = open(a.out, 'w') if a.out else sys.stdout
    for name in a.arms.split(','):
        env = {k: v for k, v in os.environ.items() if k not in FUSED}
        env.update(ARMS[name][0])
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), '--tree', tree, '--arm', name], env=env,
                               stdout=subprocess.PIPE, timeout=ARM_TIMEOUT)
        except subprocess.TimeoutExpired:
            sys.exit('arm %s: no result after %d s; stopping' % (name, ARM_TIMEOUT))
        out.write(r.stdout.decode())
        out.flush()
        if r.returncode != 0:
            sys.exit('arm %s failed (exit %d); stopping' % (name, r.returncode))
    return 0


if __name__ == '__main__':
    sys.exit(main())
