"""Host-side guard of the per-operator conv sweep (tests/conv_cases.py, tests/test_gpu_conv_ops.py): every
case is laid out as the engines lay their programs out and planned with gpi_conv_shape_plan (no device), and
the decoded shapes (conv.hip ShapeC, field names read from the source) must reach every kernel variant the
sweep exists for.  A later tile-rule change that moves a case off its variant fails here, on the CPU, instead
of silently shrinking what the GPU sweep covers: give the case another shape that reaches the variant again
(or add one), never drop the variant from the lists below."""
import pytest

from gpi import _lib as L
from conv_cases import (CASES, REFUSALS, CONV_SHAPES_H, chain, lay_out, plan_ctx, plan_shape, shape_fields,
                        parse_shapes)

GPI_ERR_UNSUPPORTED = -3


@pytest.fixture(scope='module')
def planned():
    """case id -> {'fwd' | 'bwd' | 'fuse': decoded shape of T's launch}; every other op of the chain must plan
    too (forward, and backward unless the case is forward only)."""
    lib = L.lib()
    fields = shape_fields()
    out = {}
    for case in CASES:
        prog = chain(case)
        ws, g, descs = lay_out(case, prog)
        ctx = plan_ctx(g)
        shapes = {}
        for op, d in zip(prog.ops, descs):
            passes = [('fwd', 1, 0)] + ([('bwd', 0, 0)] if case.grad else [])
            if op is prog.T and case.loss:
                passes.append(('fuse', 0, 1))
            for what, fwd, fuse in passes:
                if fuse:
                    d.out_off = -1      # as the engine: the fused loss epilogue writes no output image
                rc, s = plan_shape(lib, d, ctx, fwd, fuse, fields if op is prog.T else None)
                assert rc == 0, (case.id, op.name, what, rc)
                if op is prog.T:
                    shapes[what] = s
        out[case.id] = shapes
    return out


def test_case_ids_are_unique():
    ids = [c.id for c in CASES + REFUSALS]
    assert len(set(ids)) == len(ids)


def test_every_case_reaches_its_variants(planned):
    for case in CASES:
        for what, want in case.reach.items():
            s = planned[case.id][what]
            got = {k: s[k if k in s else 'G_' + k] for k in want}
            assert got == want, (case.id, what, got, want)


def test_refusals_are_refused():
    lib = L.lib()
    for case in REFUSALS:
        prog = chain(case)
        ws, g, descs = lay_out(case, prog)
        ctx = plan_ctx(g)
        d = descs[prog.ops.index(prog.T)]
        assert plan_shape(lib, d, ctx, 1, 0)[0] == 0, case.id      # the forward runs
        assert plan_shape(lib, d, ctx, 0, 0)[0] == GPI_ERR_UNSUPPORTED, case.id


def test_table_reaches_every_variant(planned):
    fwd = [s['fwd'] for s in planned.values()]
    bwd = [s['bwd'] for s in planned.values() if 'bwd' in s]
    fuse = [s['fuse'] for s in planned.values() if 'fuse' in s]

    def some(shapes, **kw):
        return any(all(s[k] == v for k, v in kw.items()) for s in shapes)

    for cg in (2, 3, 4):
        assert some(fwd, G_cg=cg, npxk=0), 'forward cg %d' % cg
    for npx in (1, 2, 4):
        assert some(fwd, npxk=npx), 'forward %d px / thread' % npx
    for cp in (2, 4, 6, 8):
        assert some(fwd, cp=cp), 'forward cp %d' % cp
    assert some(fwd, half=1), 'forward half tiles'
    for v in (0, 1):
        assert some(bwd, G_zreg=v, D_gout_mode=0), 'backward zreg %d' % v
        assert some(bwd, G_lsum=v), 'backward lsum %d' % v
        assert some(bwd, G_split=v, has_gin=1), 'backward split %d' % v
        assert some(bwd, D_gin_accumulate=v, has_gin=1), 'backward gin_accumulate %d' % v
        assert some(fuse, half=v), 'fused half %d' % v
    assert some(bwd, G_ucls=1, upk=2), 'backward ucls'
    assert some(bwd, G_ucls=0, D_upsample=1), 'upsampling backward without ucls'
    assert some(bwd, G_vshift=1, G_vsum=1), 'vshift with vsum'
    assert some(bwd, G_vshift=1, G_vsum=0), 'vshift without vsum'
    assert some(bwd, half=1, G_lsum=1), 'backward half tiles with lsum'
    assert some(bwd, half=1, G_split=0, has_gin=1), 'backward half tiles without split'
    assert some(bwd, D_k=5, fusek=0), 'VALU input gradient, separate launch'


def test_no_case_runs_a_compile_time_shape_kernel(planned):
    """The sweep is for the generic (SHP = -1) kernels; the shape kernels are held bit-identical to them by
    tests/test_gpu_shapes.py."""
    table = set(parse_shapes(open(CONV_SHAPES_H).read()))
    assert table
    for cid, shapes in planned.items():
        for what, s in shapes.items():
            assert s['_row'] not in table, (cid, what)
