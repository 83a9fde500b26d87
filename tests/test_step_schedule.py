"""The ELBO step's schedule table (gpi.schedule.step_schedule) over the full product of its inputs, and the
joiners that walk it (gpi.engine.EventJoiner / FlagJoiner on recording stand-ins for streams, events and the
engine; the segment joiner's order, gpi.schedule.segments).  No GPU, no native library."""
import itertools

from gpi.engine import EventJoiner, FlagJoiner
from gpi.schedule import MAIN, SIDE, E_ROM, E_DEC, E_ENC, E_SIDE, E_VALUE, segments, step_schedule, walk

INPUTS = list(itertools.product((0, 1, 11), (False, True), ('split', 'main'), ('forward', 'backward'),
                                (False, True), (False, True), (False, True), (None, 'now', 'defer')))


def rows_of(args):
    s = step_schedule(*args)
    return list(s.forward) + list(s.backward)


def per_stream(pieces):
    return {st: [p for s, p in pieces if s == st] for st in (MAIN, SIDE)}


def test_every_waited_edge_is_signalled_once_on_the_other_stream_and_earlier():
    for args in INPUTS:
        rows = rows_of(args)
        for i, r in enumerate(rows):
            if r.wait is None:
                continue
            sig = [j for j, q in enumerate(rows) if q.signal == r.wait]
            assert len(sig) == 1, (args, r)
            assert rows[sig[0]].stream != r.stream, (args, r)        # never an edge of its own stream
            assert sig[0] < i, (args, r)                             # enqueued ahead of its waiter


def test_edges_and_side_stream_end():
    for args in INPUTS:
        s = step_schedule(*args)
        rows = list(s.forward) + list(s.backward)
        edges = {e for r in rows for e in (r.wait, r.signal) if e is not None}
        assert {e for e in edges if e != E_VALUE} <= {0, 1, 2, 3}, args
        assert all(isinstance(e, int) for e in edges if e != E_VALUE)
        side = [r for r in rows if r.stream == SIDE]
        assert side[-1].signal == E_SIDE, args                       # edge 3: the side stream's last signal
        assert [r.signal for r in side].count(E_SIDE) == 1
        assert s.backward[-1] == (MAIN, None, E_SIDE, None, False, {})
        # a folded signal needs a later main-stream piece of the same half to ride on
        for half in (s.forward, s.backward):
            for i, r in enumerate(half):
                if r.fold:
                    assert r.stream == MAIN and any(q.stream == MAIN and q.piece for q in half[i + 1:]), (args, r)


class Recorder(object):
    """Stand-ins for torch streams / events and the engine: every call lands in one log, in host order."""

    class Stream(object):
        def __init__(self, name, log):
            self.name, self.log = name, log

        def wait_event(self, ev):
            self.log.append((self.name, 'wait_event', ev.edge))

    class Event(object):
        def __init__(self, edge, log):
            self.edge, self.log = edge, log

        def record(self, stream):
            self.log.append((stream.name, 'record', self.edge))

    def __init__(self):
        self.log = []
        self.streams = {k: (self.Stream(k, self.log), k) for k in (MAIN, SIDE)}     # launch handle = the name
        self.events = {k: self.Event(k, self.log) for k in (E_ROM, E_DEC, E_ENC, E_SIDE, E_VALUE, 'start')}
        self.handoff, self.side_done = True, None

    def _signal(self, k, st):
        self.log.append((st, 'signal', k))

    def _wait(self, k, st):
        self.log.append((st, 'wait', k))

    def run(self, s, sig):
        self.log.append((s.stream, 'piece', s.piece))
        if sig is not None:
            self.log.append((s.stream, 'signal', sig))               # folded into the piece's first launch

    def walk(self, args, flags, main_wait=True):
        s = step_schedule(*args)
        for k, half in enumerate((s.forward, s.backward)):
            j = EventJoiner(self.events, self.streams)
            if flags:
                j = FlagJoiner(self, j, main_wait)
            if k == 0:
                j.begin()
            walk(half, j, self.run)
            if k == 1:
                j.end()
        return self.log


def pieces(log):
    return [(st, what) for st, kind, what in log if kind == 'piece']


def test_joiners_run_the_same_pieces_per_stream():
    for args in INPUTS:
        table = per_stream([(r.stream, r.piece) for r in rows_of(args) if r.piece])
        ev, fl = Recorder().walk(args, False), Recorder().walk(args, True)
        assert per_stream(pieces(ev)) == table, args
        assert per_stream(pieces(fl)) == table, args
        # events: a wait_event ahead of its record would wait for nothing -- every wait follows its signal in
        # host order; flags: every flag waited on is signalled once (the waits spin, host order is free)
        for i, (st, kind, e) in enumerate(ev):
            if kind == 'wait_event':
                assert [s for s, k, q in ev[:i] if q == e and k == 'record'] == [SIDE if st == MAIN else MAIN], (args, e)
        assert not [x for x in ev if x[1] in ('signal', 'wait')], args
        for st, kind, e in fl:
            if kind == 'wait':
                assert [s for s, k, q in fl if q == e and k == 'signal'] == [SIDE if st == MAIN else MAIN], (args, e)


def test_flag_joiner_leaves_edge_3_to_the_epilogue_without_main_wait():
    for args in INPUTS:
        log = Recorder().walk(args, True, main_wait=False)
        assert (MAIN, 'wait', E_SIDE) not in log and (SIDE, 'signal', E_SIDE) in log, args


def test_segment_joiner_runs_the_same_pieces_per_stream():
    for args in INPUTS:
        enc, rom, enc_reduce, rom_at, rom_first, early, value, running = args
        if rom_at != 'forward' or rom_first or early or value or running != 'defer':
            continue                                                  # what segments mode supports
        rows, segs = rows_of(args), segments(step_schedule(*args))
        assert per_stream([(g.stream, r.piece) for g in segs for r in g.rows]) == \
            per_stream([(r.stream, r.piece) for r in rows]), args
        for i, g in enumerate(segs):
            assert len({r.stream for r in g.rows}) == 1
            if g.wait is not None:
                assert [q.stream for q in segs[:i] if q.signal == g.wait] == [SIDE if g.stream == MAIN else MAIN]
        assert all(g.signal != E_VALUE for g in segs)                 # nobody waits on it: not realised


def test_default_schedule_written_out():
    """(encoder, ROM, enc_reduce='split', rom_at='forward'): the fused step's default, as (stream, piece, waits on,
    signals), transcribed from ElboEngine.forward() / backward() before the table existed."""
    s = step_schedule(11, True, 'split', 'forward', False, False, False, 'defer')
    assert [r[:4] for r in s.forward] == [
        (MAIN, 'forward_a', None, E_ROM),             # encoder, head forward; flags: 0 rides on the decoder's first conv
        (MAIN, 'forward_b', None, None),              # decoder forward, fused output conv
        (SIDE, 'rom_side', E_ROM, E_VALUE),           # ROM solves, enqueued after the decoder
    ]
    assert [r[:4] for r in s.backward] == [
        (MAIN, 'backward_a', None, E_DEC),            # decoder backward, the encoder samples' head backward
        (MAIN, 'backward_b', None, E_ENC),            # encoder backward but the input conv
        (MAIN, 'backward_c', None, None),             # input conv backward, its slab reduction
        (SIDE, 'backward_side_a', E_DEC, None),       # q samples' head backward, decoder reduction, GEMM, next noise
        (SIDE, 'backward_side_b', E_ENC, E_SIDE),     # the rest of the encoder slab reduction
        (MAIN, None, E_SIDE, None),                   # the step's continuation (epilogue + Adam) behind the side's end
    ]
    assert s.backward[0].args == {'split': True} and s.backward[0].fold and s.backward[1].fold and s.forward[0].fold
    assert s.backward[3].args == {'split': True, 'rom': False, 'running': True}
    # the module path: value read after the forward, running statistics at its end, head backward not split
    m = step_schedule(11, True, 'split', 'forward', False, False, True, 'now')
    assert [r[:4] for r in m.forward] == [(MAIN, 'forward_a', None, E_ROM), (MAIN, 'forward_b', None, None),
                                          (SIDE, 'rom_side', E_ROM, E_VALUE), (MAIN, 'running_now', None, None),
                                          (MAIN, None, E_VALUE, None)]
    assert m.backward[0].args == {'split': False} and [r[:4] for r in m.backward] == [r[:4] for r in s.backward]
    # rom_at='backward': no edge 0, the ROM rides with the backward's side work
    d = step_schedule(11, True, 'split', 'backward', False, False, False, 'defer')
    assert [r[:4] for r in d.forward] == [(MAIN, 'forward_a', None, None), (MAIN, 'forward_b', None, None)]
    assert d.backward[3].args == {'split': True, 'rom': True, 'running': True}
