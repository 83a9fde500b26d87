"""CPU checks on the ROM operator sweep's case table (tests/rom_cases.py): the table reaches what it claims to
reach, its bars are attainable in fp32, and the comparison would notice the mistakes it is there to catch -- each
deliberately wrong variant of the reference (tests/rom_ref.py WRONG) differs from the right one by more than the
bar on every case tagged with that edge.  No kernel runs here; the refusals are return codes of gpi_rom's argument
checks, which come before any launch."""
import os

import numpy as np
import pytest
import torch

import rom_cases as T
import rom_ref as R


def test_case_count_and_ids():
    cs = T.cases()
    n_shapes = len(T.NATIVE_SHAPES) + len(T.GENERIC_SHAPES)
    assert n_shapes == 26 + 14 and len(T.COARSE_SHAPES) == 14
    n_opt = sum(len(T.OPTION_MODES[o]) for o in T.OPTIONS)
    assert len(cs) == 5 * n_shapes + 14 + 4 * n_opt + 4 * len(T.COARSE_OPTIONS) == 286
    assert len({c.id for c in cs}) == len(cs)
    assert [c.index for c in cs] == list(range(len(cs)))
    assert {c.family for c in cs} == set(T.FAMILIES)


def test_shapes_of_the_table():
    base = [c for c in T.cases() if c.opt is None]
    for nc in (4, 8, 16):
        got = {(c.r, c.N) for c in base if c.nc == nc and c.mode != 'coarse'}
        assert got >= {(r, N) for r in (1, 2, 3, 5) for N in (1, 3)}
        assert ((7, 3) in got) == (nc != 16)
    gen = {(c.nc, c.r) for c in base if c.family == 'generic' and c.mode != 'coarse'}
    assert gen == {(nc, r) for nc in (2, 3, 6, 7, 11, 15) for r in (1, 3)} | {(2, 2), (15, 2)}
    assert all(c.N == 2 for c in base if c.family == 'generic')
    for fam in ('lane4', 'lane8'):
        assert {c.N for c in base if c.family == fam} == {1, 63, 64, 65, 130}
    assert {c.N for c in base if c.family == 'coarse16'} == {1, 2, 3}
    assert [(c.nc, c.N) for c in base if c.family == 'generic' and c.mode == 'coarse'] == [(7, 2)]
    # every shape runs every mode
    for shape in T.NATIVE_SHAPES + T.GENERIC_SHAPES:
        assert {c.mode for c in base if (c.nc, c.r, c.N) == shape and c.mode != 'coarse'} == set(T.MODES)
    for c in T.cases():
        if c.opt == 'contrast':
            assert c.r == 2 and c.N == 5


def test_every_tag_and_every_family_mode_option():
    cs = T.cases()
    for tag in T.TAGS:
        assert any(tag in c.tags for c in cs), tag
    assert {t for c in cs for t in c.tags} == set(T.TAGS)
    have = {(c.family, c.mode, c.opt) for c in cs}
    for fam in T.FULL_FAMILIES:
        for mode in T.MODES:
            assert (fam, mode, None) in have
        for opt in T.OPTIONS:
            for mode in T.OPTION_MODES[opt]:
                assert (fam, mode, opt) in have, (fam, mode, opt)
        # the issue's pairs by name
        for pair in (('forward', 'kappa'), ('bwd_both', 'kappa'), ('loglik', 'x_draw'), ('loglik', 'gx_acc'),
                     ('loglik', 'loss_scale'), ('forward', 'flag'), ('forward', 'contrast'), ('loglik', 'contrast'),
                     ('bwd_both', 'contrast')):
            assert (fam,) + pair in have
    for fam in ('lane4', 'lane8', 'coarse16', 'generic'):
        for opt in (None,) + T.COARSE_OPTIONS:
            assert (fam, 'coarse', opt) in have, (fam, opt)
    # the edges per family: odd r, r = 1, the 0 / 1 column squares, the reciprocal divide, duc, d/dkappa
    for fam in T.FULL_FAMILIES:
        for tag in ('odd_r', 'r1', 'ncol01', 'umulhi', 'duc', 'kappa', 'kappa_eps', 'scale_value', 'no_duc'):
            assert any(tag in c.tags and c.family == fam for c in cs), (fam, tag)
    assert {c.r for c in cs if 'umulhi' in c.tags} == {3, 5, 7}
    assert {c.N for c in cs if 'ragged_wave' in c.tags and c.family == 'lane8'} >= {1, 63, 65, 130}
    assert {c.nc for c in cs if c.family == 'generic'} == {2, 3, 6, 7, 11, 15}


def test_input_statistics():
    for c in T.cases():
        d = c.inputs()
        D = c.dims
        assert d['x'].shape == (c.N, D['nT']) and d['F'].shape == (c.N, D['nn']) and d['Y'].shape == (c.N, D['dy'])
        assert all(d[k].dtype == np.float32 for k in ('x', 'F', 'Y', 'ls', 'dmu', 'duc'))
        interior = [e for e in range(D['nn']) if e % (c.nc + 1) not in (0, c.nc)]
        assert (d['F'][:, interior] == 0).all() and np.abs(d['F']).max() <= 0.5
        assert abs(d['ls'].mean() - np.log(0.3)) < 0.15
        if c.input_kappa:
            assert d['x'].min() > (1e-12 if c.opt != 'kappa_tiny' else 1e-11)
            assert (d['x'].max() < 1e-5) == (c.opt == 'kappa_tiny')
        elif c.opt == 'contrast':
            assert 1.0 < d['x'].std() < 2.0
        else:
            assert np.abs(d['x']).max() < 0.3 + 5 * 0.7 + 0.1
        if c.opt == 'x_draw':
            assert set(np.unique(d['x_ls'])) == {0.0, -np.inf}
            want = np.where(d['x_ls'] == 0, d['x_mu'].astype(np.float64) + d['x_eps'].astype(np.float64),
                            d['x_mu'].astype(np.float64)).astype(np.float32)
            assert np.array_equal(d['x'], want)
    # the modes of a shape share their inputs; shapes do not
    a, b = T.select('fast8', 'forward')[0], T.select('fast8', 'loglik')[0]
    assert (a.nc, a.r, a.N) == (b.nc, b.r, b.N) and a.inputs() is b.inputs()
    assert not np.array_equal(T.select('fast8', 'forward')[2].inputs()['x'][0], a.inputs()['x'][0])


def test_bars_are_attainable_in_fp32():
    """The reference evaluated in fp32 (dense torch solve) stays within a quarter of the bars of its fp64 self."""
    worst = {}
    for c in T.cases():
        errs = T.compare(c.evaluate(torch.float32), c.reference())
        for k, e in errs.items():
            assert e <= 0.25 * T.BAR[k], (c.id, k, e)
            if k == 'uc' and c.nc in (4, 8):      # coarse-only vs full forward: two fp32 solves, half CROSS_BAR each
                assert e <= 0.5 * T.CROSS_BAR, (c.id, k, e)
            if e > worst.get(k, (0.0, None))[0]:
                worst[k] = (e, c.id)
    print('fp32 dense solve vs fp64, worst per quantity:', worst)
    assert set(T.DRAW) <= {(c.nc, c.r, c.N, c.opt) for c in T.cases() if c.opt == 'contrast'}


@pytest.mark.parametrize('wrong', R.WRONG)
def test_comparator_notices(wrong):
    cs = [c for c in T.cases() if wrong in c.tags]
    assert len(cs) >= 4, len(cs)
    assert {c.family for c in cs} >= set(T.FULL_FAMILIES)
    for c in cs:
        errs = T.compare(c.evaluate(wrong=wrong), c.reference())
        assert T.over_bar(errs), (c.id, wrong, errs)


def test_comparator_passes_the_reference_itself():
    for c in T.cases()[::37]:
        errs = T.compare(c.evaluate(), c.reference())
        assert not T.over_bar(errs) and max(errs.values()) == 0.0


def test_the_flag_case_would_raise_in_the_reference():
    """The poked kappa of the flag cases is what ROM.__call__ refuses (kappa <= 1e-12)."""
    c = next(c for c in T.cases() if c.opt == 'flag')
    d = c.inputs()
    k = d['x'].copy()
    k[d['poke']] = 1e-13
    with pytest.raises(ValueError):
        R.forward(c.nc, c.r, k, d['F'], input_kappa=True)


def test_refusals_are_return_codes():
    """gpi_rom's argument checks (no launch, so no GPU): nc = 1, 17, refine = 0, LOGLIK without Y / logsig_y /
    both gradient sinks / gx, BACKWARD without dmu and duc / without gx; n = 0 is accepted."""
    import ctypes as C
    from gpi import _lib as L
    if not os.path.exists(L.LIB_PATH):
        pytest.skip('libgpi_hip.so is not built')
    lib, OK, ERR_ARG = L.lib(), 0, -1
    buf = (C.c_float * 4096)()
    p = C.cast(buf, C.c_void_p).value

    def desc(mode, **kw):
        r = L.RomDesc()
        r.nc, r.refine, r.n, r.mode = 4, 2, 0, mode
        for k in ('x', 'F', 'Y', 'logsig_y', 'gx', 'gls_part', 'gacc_logsig', 'dmu', 'duc', 'mu_y', 'uc'):
            setattr(r, k, p)
        r.x_stride = r.gx_stride = 32
        for k, v in kw.items():
            setattr(r, k, v)
        return lib.gpi_rom(C.byref(r), None)

    for mode in (L.ROM_FORWARD, L.ROM_LOGLIK, L.ROM_BACKWARD):
        assert desc(mode) == OK                      # n = 0
        assert desc(mode, nc=1) == ERR_ARG and desc(mode, nc=17) == ERR_ARG
        assert desc(mode, refine=0) == ERR_ARG
        assert desc(mode, n=-1) == ERR_ARG
        assert desc(mode, x=None) == ERR_ARG and desc(mode, F=None) == ERR_ARG
    for k in ('Y', 'logsig_y', 'gx'):
        assert desc(L.ROM_LOGLIK, **{k: None}) == ERR_ARG, k
    assert desc(L.ROM_LOGLIK, gls_part=None) == OK and desc(L.ROM_LOGLIK, gacc_logsig=None) == OK
    assert desc(L.ROM_LOGLIK, gls_part=None, gacc_logsig=None) == ERR_ARG
    assert desc(L.ROM_BACKWARD, dmu=None) == OK and desc(L.ROM_BACKWARD, duc=None) == OK
    assert desc(L.ROM_BACKWARD, dmu=None, duc=None) == ERR_ARG
    assert desc(L.ROM_BACKWARD, gx=None) == ERR_ARG
    assert all(v == 0 for v in buf)
