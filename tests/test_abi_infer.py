"""C ABI of the inference entry points without a GPU: argument errors return a code and launch
nothing; the eval layout of the codec programs (host-side planning only)."""
import ctypes as C
import os

import pytest


@pytest.fixture(scope='module')
def lib():
    from gpi import _lib as L
    if not os.path.exists(L.LIB_PATH):
        pytest.fail('libgpi_hip.so is not built (run __graft_entry__.build())')
    return L


def test_bn_eval_seed_rejects_null_and_empty_arguments(lib):
    L = lib.lib()
    items = (lib.BnEvalItem * 2)()
    stats = (lib.Stat * 8)()
    ip, sp = C.cast(items, C.c_void_p), C.cast(stats, C.c_void_p)
    assert L.gpi_bn_eval_seed(None, 2, 4, sp, 8, None) == -1
    assert L.gpi_bn_eval_seed(ip, 2, 4, None, 8, None) == -1
    assert L.gpi_bn_eval_seed(ip, 0, 4, sp, 8, None) == -1
    assert L.gpi_bn_eval_seed(ip, -1, 4, sp, 8, None) == -1
    assert L.gpi_bn_eval_seed(ip, 2, 0, sp, 8, None) == -1
    assert L.gpi_bn_eval_seed(ip, 2, 4, sp, 0, None) == -1
    assert all(s.sum == 0.0 and s.sumsq == 0.0 for s in stats)


def test_affine_rejects_null_and_empty_arguments(lib):
    L = lib.lib()
    buf = (C.c_float * 16)()
    p = C.cast(buf, C.c_void_p)
    assert L.gpi_affine(None, p, p, p, 1, 2, 2, None) == -1
    assert L.gpi_affine(p, p, None, p, 1, 2, 2, None) == -1
    assert L.gpi_affine(p, p, p, None, 1, 2, 2, None) == -1
    assert L.gpi_affine(p, p, p, p, 0, 2, 2, None) == -1
    assert L.gpi_affine(p, p, p, p, 1, 0, 2, None) == -1
    assert L.gpi_affine(p, p, p, p, 1, 2, 0, None) == -1


def test_bn_eval_item_layout(lib):
    assert C.sizeof(lib.BnEvalItem) == 40
    assert lib.BnEvalItem.count.offset == 16 and lib.BnEvalItem.running_mean.offset == 24


@pytest.mark.parametrize('n', [64, 1024, 288 * 4096])
def test_seeding_identity_in_fp64(n):
    """The arithmetic of gpi_bn_eval_seed followed by the kernels' bn_mean_invstd, restated in fp64 on the
    host: sum = n m, sumsq = n (v + m^2) give back m bit for bit and 1 / sqrt(v + eps) with no difference
    after the cast to fp32 (|mean| up to 9, var >= 1e-3)."""
    import numpy as np
    rng = np.random.default_rng(n)
    m = (rng.uniform(-9, 9, 4096)).astype(np.float32)
    v = (1e-3 + rng.uniform(0, 4, 4096) ** 2).astype(np.float32)
    m64, v64, nn = m.astype(np.float64), v.astype(np.float64), np.float64(n)
    s, s2 = nn * m64, nn * (v64 + m64 * m64)
    mean = s / nn
    var = np.maximum(s2 / nn - mean * mean, 0.0)
    assert np.array_equal(mean.astype(np.float32), m) and np.array_equal(mean, m64)
    inv = (1.0 / np.sqrt(var + np.float64(np.float32(1e-5)))).astype(np.float32)
    want = (1.0 / np.sqrt(v64 + np.float64(np.float32(1e-5)))).astype(np.float32)
    assert np.array_equal(inv, want)


@pytest.mark.parametrize('kind', ['encoder', 'decoder'])
def test_eval_layout_gives_every_bn_its_own_records(lib, kind):
    """plan.layout(eval_mode=True): per-layer stat ranges that do not overlap, no statistics epilogue,
    no dropout, no backward buffers or slabs; the train layout of the same program is unchanged."""
    from gpi import plan
    from gpi.plan import Arena

    def build():
        if kind == 'encoder':
            return plan.encoder_program(64, [1, 2, 1], 4, 6, drop_rate=0.2)
        return plan.decoder_program(8, 1, 6, [1, 2, 1], 4, drop_rate=0.2)

    g = lib.Groups()
    g.n_groups = 1
    for i in range(1, lib.GPI_MAX_GROUPS + 1):
        g.start[i] = 3
    offs = {}
    off = lambda n: offs.setdefault(n, 1000 * len(offs))
    pe, ws, st, parts = build(), Arena(), Arena(align=1), Arena()
    descs = pe.layout(3, ws, st, parts, g, off, eval_mode=True)
    ranges = []
    for op, d in zip(pe.ops, descs):
        assert d.epilogue == lib.EPI_STORE and d.out_stat == -1 and d.drop_off == -1
        assert d.wpart_off == -1 and d.gout_off == -1 and d.gin_off == -1
        if op.bn is None:
            assert d.in_bn == 0 and d.in_stat == -1
        else:
            assert d.in_bn == 1
            ranges.append((d.in_stat, d.in_stat + op.cin))
    ranges.sort()
    assert ranges[0][0] == 0 and ranges[-1][1] == st.size
    assert all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))
    assert st.size == sum(op.cin for op in pe.ops if op.bn is not None)
    assert parts.size == 0 and pe.drop_numel == 0
    assert all(b.s_off is None for b in pe.buffers)
    # the train layout still shares one record per block-buffer channel and keeps the backward buffers
    pt, ws_t, st_t, parts_t = build(), Arena(), Arena(align=1), Arena()
    descs_t = pt.layout(3, ws_t, st_t, parts_t, g, off)
    assert st_t.size == sum(b.C for b in pt.buffers if b.bn_consumed) < st.size
    assert any(d.epilogue == lib.EPI_STORE_STATS for d in descs_t) and pt.drop_numel > 0
    assert ws_t.size > ws.size and parts_t.size > 0
