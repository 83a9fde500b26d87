"""The ELBO training step's two-stream schedule, as data.

step_schedule() is the one place that says which piece of the step (an ElboEngine method) runs after which, on
which stream, behind which cross-stream edge.  It is a pure function of the facts that decide the schedule: no
torch, no GPU.  The joiners (gpi.engine.EventJoiner / FlagJoiner, FusedElboStep's segment graphs) walk its rows
and state only how an edge is realised.

Edges keep the hand-off flag numbers (fixed from outside: the fused epilogue's wait_flag reads word 3, the
error word sits at index 4):
    0 E_ROM    head forward -> ROM
    1 E_DEC    decoder and head backward done
    2 E_ENC    encoder backward except the input conv done
    3 E_SIDE   the side stream's end
    E_VALUE    the forward's ROM done, for a value read right after the forward (always an event)
The step-start gate (the side stream's step begins after the main stream's previous step) orders steps, not
stretches of one step: it belongs to the joiners' begin(), not to a row.
"""
from collections import namedtuple
from functools import lru_cache

MAIN, SIDE = 'main', 'side'
E_ROM, E_DEC, E_ENC, E_SIDE = 0, 1, 2, 3
E_VALUE = 'value'

# One stretch of a stream between two cross-stream edges: wait (edge or None) -> piece (ElboEngine method name, or
# None: the step's continuation on that stream) -> signal (edge or None).  fold: the flag joiner may fold the signal
# into the first conv launch of the main stream's next piece (the *_sig entry points) instead of a launch of its
# own; False where that piece has no conv to carry it.  args: the piece's keyword arguments the table decides.
Stretch = namedtuple('Stretch', 'stream piece wait signal fold args')
Schedule = namedtuple('Schedule', 'forward backward')
Segment = namedtuple('Segment', 'stream rows wait signal')


def _row(stream, piece, wait=None, signal=None, fold=False, **args):
    return Stretch(stream, piece, wait, signal, fold, args)


@lru_cache(maxsize=None)
def step_schedule(enc_convs, rom, enc_reduce='split', rom_at='forward', rom_first=False, early=False,
                  compute_value=False, running=None):
    """(forward rows, backward rows) in enqueue order.
    enc_convs: convs of the encoder program (0: no encoder); rom: the step has ROM launches; enc_reduce 'split' /
    'main'; rom_at 'forward' / 'backward'; rom_first; early: the ROM at the very start of the step (behind the
    step gate alone); compute_value: the value is read after the forward; running: BN running statistics 'now'
    (end of the forward), 'defer' (with the backward's side work) or None."""
    rom = bool(rom)
    # rom_at 'backward': the ROM follows the backward's fork on the side stream (ahead of the variational
    # samples' head backward that needs it) -- one cross-stream dependency less per step; only when the value is
    # not read right after the forward
    deferred = rom and rom_at == 'backward' and not compute_value
    in_forward = rom and not deferred
    early = bool(early) and in_forward
    fork = in_forward and not early
    # The ROM solve only feeds the head backward: it runs on the side stream, concurrently with the decoder.
    rom_row = _row(SIDE, 'rom_side', wait=E_ROM if fork else None, signal=E_VALUE)
    fwd = [rom_row] if early else []
    fwd.append(_row(MAIN, 'forward_a', signal=E_ROM if fork else None, fold=fork))
    if fork and rom_first:
        fwd.append(rom_row)
    # The decoder is enqueued ahead of the ROM (rom_first False) so that, in a captured graph, the main chain is
    # the fork's first branch and keeps its hardware queue (each cross-queue dependency costs ~10 us).
    fwd.append(_row(MAIN, 'forward_b'))
    if fork and not rom_first:
        fwd.append(rom_row)
    if running == 'now':
        fwd.append(_row(MAIN, 'running_now'))
    if compute_value and in_forward:
        fwd.append(_row(MAIN, None, wait=E_VALUE))

    # The split rule: with the ROM still pending on the side stream, only the encoder samples' head backward
    # runs on the main stream; the variational samples' (which need the ROM adjoint) follow the ROM on the side
    # stream, so the main chain never waits for the ROM.
    split = rom and not compute_value
    enc = enc_convs > 0
    enc_split = enc and enc_reduce == 'split'
    # flags: the encoder backward's first conv signals 1 (the head backward is done), the input conv's
    # backward 2 (the rest of the encoder backward is done)
    bwd = [_row(MAIN, 'backward_a', signal=E_DEC, fold=enc_convs > 1, split=split)]
    if enc:
        bwd.append(_row(MAIN, 'backward_b', signal=E_ENC if enc_split else None, fold=enc_split))
        bwd.append(_row(MAIN, 'backward_c', enc_split=enc_split))
    # The decoder's slab reduction and the dense weight gradients depend only on what is done after backward_a:
    # they run on the side stream, concurrently with the encoder backward -- and are enqueued after it, so the
    # encoder stays on the main chain's queue in a graph (captured ahead of the encoder backward instead, the side
    # branch took the launch stream and the main chain the pooled one: 0.7526 vs 0.6289 ms per step, r03).
    bwd.append(_row(SIDE, 'backward_side_a', wait=E_DEC, signal=None if enc_split else E_SIDE, split=split,
                    rom=deferred, running=running == 'defer'))
    if enc_split:
        bwd.append(_row(SIDE, 'backward_side_b', wait=E_ENC, signal=E_SIDE))
    bwd.append(_row(MAIN, None, wait=E_SIDE))
    return Schedule(tuple(fwd), tuple(bwd))


def walk(rows, joiner, run):
    """Enqueue rows in order: joiner.wait(edge, stream) / run(row, sig) / joiner.signal(edge, stream, fold).  A
    signal the joiner folds (it returns the flag number) rides on the main stream's next piece as run's sig."""
    pending = None
    for s in rows:
        if s.wait is not None:
            joiner.wait(s.wait, s.stream)
        if s.piece is not None:
            sig = None
            if s.stream == MAIN:
                sig, pending = pending, None
            run(s, sig)
        if s.signal is not None:
            folded = joiner.signal(s.signal, s.stream, s.fold)
            pending = folded if folded is not None else pending
    assert pending is None, 'a folded signal found no main-stream piece to carry it'


def waited(rows):
    return {s.wait for s in rows if s.wait is not None}


def segments(sched):
    """The whole step as single-stream graph segments, in the segment joiner's replay order: every stretch its
    own segment, a side stretch right behind the stretch that signals the edge it waits on (each graph is launched
    as early as its edge allows; the other joiners enqueue the side work after the encoder backward), and the
    two main stretches across the forward / backward seam, which no edge separates, as one.  Signals nobody
    waits on (E_VALUE when the value is not read) are dropped."""
    rows = list(sched.forward) + list(sched.backward)
    used = waited(rows)
    order = [s for s in rows if s.stream == MAIN or s.wait is None]
    for s in rows:
        if s.stream == SIDE and s.wait is not None:
            at = max(i for i, r in enumerate(order) if r.signal == s.wait or r.stream == SIDE)
            order.insert(at + 1, s)
    seam = [s for s in sched.forward if s.stream == MAIN][-1], sched.backward[0]
    out = []
    for s in order:
        sig = s.signal if s.signal in used else None
        if s is seam[1] and out and out[-1].rows[-1] is seam[0] and out[-1].signal is None and s.wait is None:
            out[-1] = Segment(s.stream, out[-1].rows + (s,), out[-1].wait, sig)
        else:
            out.append(Segment(s.stream, (s,), s.wait, sig))
    return out
