"""gpi_param_norms on a synthetic flat buffer against numpy fp64: per-segment 2-norms, their sum in segment order
and the penalty's gradient lambda p / ||p||, for segments of 1 .. 65 536 floats at odd offsets with unpenalised
floats between them.

Bars: norms and their sum 1e-14 relative (fp64 sums of exact squares: at most 64 + 6 + 16 additions deep per
element at 65 536 floats, each within 2^-53; the square root halves the relative error); the gradient 3 * 2^-24
relative (one fp32 rounding of the result, plus slack for a form that rounds the coefficient and the product)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 4, 63, 64, 65, 255, 256, 257, 4097, 65536, 7, 1]     # [-2]: the all-zero segment, [-1]: one negative value
ZERO_SEG, NEG_SEG = len(SIZES) - 2, len(SIZES) - 1
GRAD_SENTINEL, NORM_SENTINEL = -7777.0, -5555.0
LAM = 0.05


def layout():
    """(p, rows): fp32 buffer with NaN in every unpenalised float (a read of one would poison a norm)."""
    rng = np.random.default_rng(20261021)
    rows, off = [], 0
    for k, n in enumerate(SIZES):
        gap = 1 + k % 5                       # 1 .. 5 unpenalised floats ahead of every segment
        if (off + gap) % 2 == 0:
            gap += 1 if gap < 5 else -1       # odd offsets: never 8- or 16-byte aligned
        off += gap
        rows.append((off, n))
        off += n
    total = off + 3
    p = np.full(total, np.nan, dtype=np.float32)
    for k, (o, n) in enumerate(rows):
        p[o:o + n] = (rng.normal(size=n) * 10.0 ** rng.uniform(-3, 3, size=n)).astype(np.float32)
    o, n = rows[ZERO_SEG]
    p[o:o + n] = 0.0
    p[rows[NEG_SEG][0]] = -3.25
    return p, rows


class Case(object):
    def __init__(self, lam=LAM):
        from gpi import _lib as L
        self.L = L
        self.p_host, self.rows = layout()
        tab = [v for r in self.rows for v in r]
        self.seg_host = (C.c_int64 * len(tab))(*tab)
        self.pen_n = self.rows[-1][0] + self.rows[-1][1]
        dev = 'cuda'
        self.p = torch.tensor(self.p_host, device=dev)
        self.seg = torch.tensor(tab, dtype=torch.int64, device=dev)
        self.lam = torch.tensor([lam], dtype=torch.float32, device=dev)
        self.norms = torch.full((len(self.rows),), NORM_SENTINEL, dtype=torch.float64, device=dev)
        self.pen = torch.full((2,), NORM_SENTINEL, dtype=torch.float64, device=dev)
        self.pen_grad = torch.full((self.p.numel(),), GRAD_SENTINEL, dtype=torch.float32, device=dev)
        self.done = torch.zeros(1, dtype=torch.int32, device=dev)

    def desc(self, **over):
        k = dict(p=self.p.data_ptr(), seg=self.seg.data_ptr(), seg_host=C.addressof(self.seg_host),
                 n_seg=len(self.rows), pen_n=self.pen_n, lam=self.lam.data_ptr(), norms=self.norms.data_ptr(),
                 pen=self.pen.data_ptr(), pen_grad=self.pen_grad.data_ptr(), done=self.done.data_ptr())
        k.update(over)
        return self.L.ParamNormsDesc(**k)

    def launch(self, **over):
        d = self.desc(**over)
        rc = self.L.lib().gpi_param_norms(C.byref(d), self.L.stream_handle())
        torch.cuda.synchronize()
        return rc

    def outputs(self):
        return self.norms.cpu().numpy().copy(), self.pen.cpu().numpy().copy(), self.pen_grad.cpu().numpy().copy()


def reference(p, rows, lam32):
    norms = np.array([math.sqrt(math.fsum((p[o:o + n].astype(np.float64) ** 2).tolist())) for o, n in rows])
    pen = 0.0
    for v in norms:
        pen += v
    grads = [np.zeros(n) if nv == 0.0 else float(lam32) * p[o:o + n].astype(np.float64) / nv
             for (o, n), nv in zip(rows, norms)]
    return norms, pen, grads


def check(case, lam):
    lam32 = np.float32(lam)
    norms, pen, grad = case.outputs()
    ref_n, ref_pen, ref_g = reference(case.p_host, case.rows, lam32)
    assert np.isfinite(norms).all() and np.isfinite(pen).all()
    assert ref_n[ZERO_SEG] == 0.0 and norms[ZERO_SEG] == 0.0
    assert norms[NEG_SEG] == 3.25
    nz = ref_n > 0
    err_n = np.abs(norms[nz] - ref_n[nz]) / ref_n[nz]
    print('norms: worst relative error %.2e; pen %.2e' % (err_n.max(), abs(pen[0] - ref_pen) / ref_pen))
    assert err_n.max() <= 1e-14, err_n
    assert abs(pen[0] - ref_pen) <= 1e-14 * ref_pen
    assert abs(pen[1] - float(lam32) * ref_pen) <= 1e-14 * abs(float(lam32) * ref_pen) + 0.0
    touched = np.zeros(grad.size, dtype=bool)
    worst = 0.0
    for k, ((o, n), g) in enumerate(zip(case.rows, ref_g)):
        got = grad[o:o + n].astype(np.float64)
        touched[o:o + n] = True
        assert np.isfinite(got).all(), k
        if k == ZERO_SEG:
            assert (got == 0.0).all()
            continue
        m = g != 0.0
        assert (got[~m] == 0.0).all()
        rel = np.abs(got[m] - g[m]) / np.abs(g[m])
        worst = max(worst, rel.max())
        assert rel.max() <= 3 * 2.0 ** -24, (k, rel.max())
    print('pen_grad: worst relative error %.2e (bar %.2e)' % (worst, 3 * 2.0 ** -24))
    assert grad[case.rows[NEG_SEG][0]] < 0
    assert (grad[~touched] == np.float32(GRAD_SENTINEL)).all(), 'a float outside the segments was written'
    assert int(case.done.item()) == 0


def test_param_norms_against_numpy_fp64(device):
    case = Case()
    assert sorted(SIZES[:11]) == [1, 3, 4, 63, 64, 65, 255, 256, 257, 4097, 65536]
    assert all(o % 2 == 1 for o, _ in case.rows)
    gaps = [case.rows[k][0] - (case.rows[k - 1][0] + case.rows[k - 1][1]) for k in range(1, len(case.rows))]
    assert all(1 <= g <= 5 for g in gaps) and len(set(gaps)) >= 4 and np.isnan(case.p_host[0])
    assert case.launch() == 0
    check(case, LAM)
    first = case.outputs()
    # a second launch on the same inputs: the same bits (and the arrival counter was left at zero)
    case.norms.fill_(NORM_SENTINEL)
    case.pen.fill_(NORM_SENTINEL)
    assert case.launch() == 0
    second = case.outputs()
    for a, b in zip(first, second):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    # the factor is read from the device at launch: an edit is followed without a new descriptor
    case.lam.fill_(0.4)
    assert case.launch() == 0
    check(case, 0.4)
    third = case.outputs()
    assert np.array_equal(third[0], first[0]) and third[1][0] == first[1][0] and third[1][1] != first[1][1]
    case.lam.fill_(0.0)
    assert case.launch() == 0
    _, pen, grad = case.outputs()
    assert pen[1] == 0.0 and all((grad[o:o + n] == 0.0).all() for o, n in case.rows)


def test_param_norms_in_a_captured_graph(device):
    """Graph-capturable, and a replay follows the device factor."""
    case = Case()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        assert case.launch() == 0
    torch.cuda.current_stream().wait_stream(s)
    eager = case.outputs()
    case.pen_grad.fill_(GRAD_SENTINEL)
    g = torch.cuda.CUDAGraph()
    d = case.desc()
    with torch.cuda.graph(g):
        assert case.L.lib().gpi_param_norms(C.byref(d), case.L.stream_handle()) == 0
    g.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, case.outputs()):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    case.lam.fill_(0.4)
    g.replay()
    torch.cuda.synchronize()
    check(case, 0.4)


def test_param_norms_refusals(device):
    case = Case()
    L = case.L
    assert case.launch(n_seg=0) == -1 and case.launch(n_seg=-3) == -1
    for f in ('p', 'seg', 'seg_host', 'lam', 'norms', 'pen', 'pen_grad', 'done'):
        assert case.launch(**{f: None}) == -1, f
    assert L.lib().gpi_param_norms(None, L.stream_handle()) == -1

    def with_table(rows):
        tab = [v for r in rows for v in r]
        host = (C.c_int64 * len(tab))(*tab)
        return case.launch(seg_host=C.addressof(host), n_seg=len(rows))

    assert with_table([(-1, 4)]) == -1                              # a negative offset
    assert with_table([(3, 0)]) == -1 and with_table([(3, -2)]) == -1
    assert with_table([(case.pen_n - 3, 4)]) == -1                  # ends past pen_n
    assert with_table([(1, 2 ** 62), (5, 2)]) == -1
    assert case.launch(pen_n=0) == -1
    # nothing was launched: every output still holds its sentinel
    norms, pen, grad = case.outputs()
    assert (norms == NORM_SENTINEL).all() and (pen == NORM_SENTINEL).all() and (grad == np.float32(GRAD_SENTINEL)).all()
    assert L.lib().gpi_error_string(-1).decode() == 'invalid argument'
