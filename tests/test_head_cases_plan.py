"""CPU checks on the dense-head sweep's case table (tests/head_cases.py): the table reaches what it claims to
reach, its bars are attainable in fp32, and the comparison would notice the mistakes it is there to catch -- each
deliberately wrong variant of the reference (tests/head_ref.py WRONG) differs from the right one by more than the
bar on every case tagged with that edge.  No kernel runs here; gpi_head_form is a host-only query."""
import os

import numpy as np
import pytest
import torch

import head_cases as H
import head_ref as R


@pytest.fixture(scope='module')
def forms():
    """case id -> gpi_head_form under default dispatch (skips without the built library)."""
    from gpi import _lib as L
    if not os.path.exists(L.LIB_PATH):
        pytest.skip('libgpi_hip.so is not built')
    import ctypes as C
    lib = L.lib()
    return {c.id: lib.gpi_head_form(C.byref(c.desc(L, 4096)), 1) for c in H.cases()}


def test_case_count_and_ids():
    cs = H.cases()
    assert len(cs) == 208 == 26 * len(H.LAYOUTS)
    assert len({c.id for c in cs}) == len(cs)
    for c in cs:
        if c.mode in ('enc_engine', 'dec_engine'):
            assert c.n_q == c.n_q2 == 0
    # the issue's counts all appear, in every mode they have a meaning in
    assert {c.counts for c in cs if c.mode == 'freeX'} == set(H.COUNTS)


def test_scales_and_value_ranges():
    s = list(H.SCALES.values())
    assert len(set(s)) == 5 and all(v != 1 for v in s)
    for c in H.cases():
        for k in ('gp_ls', 'qz_ls', 'qx_ls', 'qz_ls2', 'qx_ls2'):
            v = c.params[k]
            assert v.size == 0 or (-1.5 <= v.min() and v.max() <= 0.5)
        assert -1.5 <= c.inputs['zls'].min() and c.inputs['zls'].max() <= 0.5
        assert max(np.abs(v).max() for v in c.params.values() if v.size) < 8


def test_layout_guards_and_alignment():
    """>= 8 guard floats after every workspace region and parameter block; gp_w = 2 mod 4 in the one layout."""
    for c in H.cases():
        P, ws = c.param_vector(), c.workspace()
        for regs, flat in ((c.p_reg, P), (c.w_reg, ws)):
            ends = sorted((r.off, r.off + max(r.size, 1)) for r in regs.values())
            for (a0, a1), (b0, _) in zip(ends, ends[1:] + [(len(flat), None)]):
                assert b0 - a1 >= H.NG
                assert (flat[a1:b0].view(np.uint32) == H.GUARD_BITS).all()
        assert c.p_reg['gp_w'].off % 4 == (2 if c.layout.endswith('gpw2') else 0)
        assert all(r.off % 4 == 0 for k, r in c.w_reg.items())
        # rows a mode must not write start as the pattern
        for k in ('gfeat', 'hpre', 'dhpre', 'lat', 'xs', 'mux', 'gmux', 'dzmu'):
            assert (c.w_reg[k].view(ws).view(np.uint32) == H.GUARD_BITS).all()


def test_form_coverage(forms):
    """gpi_head_form agrees with the table, and every form 0..3 is reached by >= 10 cases."""
    for c in H.cases():
        assert forms[c.id] == c.form, c.id
    for f in range(4):
        assert sum(1 for c in H.cases() if forms[c.id] == f) >= 10, f


def test_form_query_arms(forms):
    import ctypes as C
    from gpi import _lib as L
    lib = L.lib()
    for c in H.cases():
        d = c.desc(L, 4096)
        assert lib.gpi_head_form(C.byref(d), 0) == min(c.form, 1), c.id       # no prefetch: the generic form
        assert lib.gpi_head_form(C.byref(c.desc(L, 4096, L.HEAD_VALU)), 1) == 0
    d = H.cases()[0].desc(L, 0)
    assert lib.gpi_head_form(C.byref(d), 1) < 0                               # a descriptor the launchers refuse
    # the alignment gate covers gp_w only when a segment carries the gp term
    c = next(c for c in H.cases() if c.layout.endswith('gpw2') and c.mode == 'dec_engine')
    d = c.desc(L, 4096)
    assert lib.gpi_head_form(C.byref(d), 1) == 1 == c.form
    d.lat_w += 2
    assert lib.gpi_head_form(C.byref(d), 1) == 0
    c = next(c for c in H.cases() if c.layout.endswith('gpw2') and c.mode == 'holdoff' and c.n_q)
    d = c.desc(L, 4096)
    assert lib.gpi_head_form(C.byref(d), 1) == 0 == c.form
    d.gp_w += 2
    assert lib.gpi_head_form(C.byref(d), 1) == 1


def test_tile_coverage():
    """Per MFMA form: a mixed-segment tile at tile index >= 1, and a partial encoder tile after a full one."""
    for f in (1, 2, 3):
        cs = [c for c in H.cases() if c.form == f]
        assert any(c.mixed_tile >= 1 for c in cs), f
        assert any(c.partial_enc_after_full and (c.flags & R.ENC) for c in cs), f
        # ... also with segments whose flags differ, and with an empty first segment
        assert any(c.mixed_tile >= 1 and c.mode == 'holdoff' for c in cs), f
        assert any(c.n_q == 0 and c.n_q2 > 0 for c in cs), f


def test_relu_margin():
    n = 0
    for c in H.cases():
        hp = c.reference()['hpre']
        if c.n_enc and (c.flags & R.ENC):
            assert not np.isnan(hp).any()
            assert np.abs(hp).min() >= H.RELU_MARGIN, c.id
            assert (hp < 0).any() and (hp > 0).any()
            n += 1
    assert n >= 100


def test_bars_are_attainable_in_fp32():
    """The reference evaluated in fp32 stays within a quarter of the bars of its fp64 self, on every case."""
    for c in H.cases():
        errs = H.compare(R.head_reference(c, torch.float32), c.reference(), same_rows=True)
        for k, e in errs.items():
            assert e <= 0.25 * H.BAR[H.region_class(k)], (c.id, k, e)


@pytest.mark.parametrize('wrong', R.WRONG)
def test_comparator_notices(wrong):
    cs = [c for c in H.cases() if wrong in c.tags]
    assert len(cs) >= 16, len(cs)
    assert {c.layout for c in cs} == set(H.LAYOUTS)
    for c in cs:
        errs = H.compare(R.head_reference(c, wrong=wrong), c.reference(), same_rows=True)
        assert H.over_bar(errs), (c.id, wrong)


def test_comparator_passes_the_reference_itself():
    c = H.cases()[2]
    assert not H.over_bar(H.compare(R.head_reference(c), c.reference(), same_rows=True))


def test_gemm_case_table():
    gs = H.gemm_cases()
    assert len(gs) == 5 * 4 * 2 * 2 + 1 and len(gs[-1].items) == 4
    assert {(i['S'], i['M'], i['N']) for g in gs[:-1] for i in g.items} == \
        {(S, M, N) for S in H.GEMM_S for M, N in H.GEMM_MN}
    for g in gs:
        ref = g.reference()
        for k, it in enumerate(g.items):
            c = g.g_reg['c%d' % k].view(ref)
            assert np.abs(c).max() > 0 or (it['relu'] and it['S'] * it['N'] == 1)    # one clipped entry
            # fp32 evaluation of the same sums: within a quarter of the gradient bar
            A = np.stack([g.ws[it['a_off'] + s * it['lda']:][:it['M']] for s in range(it['S'])])
            B = np.stack([g.ws[it['b_off'] + s * it['ldb']:][:it['N']] for s in range(it['S'])])
            c32 = A.T @ (np.maximum(B, 0) if it['relu'] else B)
            assert R.rel_err(c32, c) <= 0.25 * H.BAR['grad']
