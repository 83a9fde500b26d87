"""Energy virtual observables without a GPU: the temperature schedules (reference
VirtualObservables.py:1040-1091, quirks included), the host form query and the argument checks of
gpi_vo_energy (nothing is launched)."""
import ctypes as C
import os

import numpy as np
import pytest


@pytest.fixture(scope='module')
def lib():
    from gpi import _lib as L
    if not os.path.exists(L.LIB_PATH):
        pytest.fail('libgpi_hip.so is not built (run __graft_entry__.build())')
    return L


@pytest.fixture(scope='module')
def VO():
    from bottleneck import VirtualObservables
    return VirtualObservables


# ---------------------------------------------------------------- schedules
def test_linear_schedule_values(VO):
    s = VO.LinearTemperatureSchedule(2.0, 0.5, 7)
    assert isinstance(s, VO.TemperatureSchedule)
    assert s.get_temperature(0) == 2.0
    assert s.get_temperature(3) == pytest.approx(2.0 + 3 / 6 * (0.5 - 2.0), rel=1e-15)
    assert s.get_temperature(6) == pytest.approx(0.5, rel=1e-15)
    # quirk: frac = it / (num_steps - 1), and it == num_steps still answers (one step past T_final)
    assert s.get_temperature(7) == pytest.approx(2.0 + 7 / 6 * (0.5 - 2.0), rel=1e-15)


def test_exponential_schedule_values(VO):
    s = VO.ExponentialTemperatureSchedule(1.0, 0.05, 4)
    assert s.get_temperature(0) == 1.0
    assert s.get_temperature(1) == pytest.approx(0.05 ** (1 / 3), rel=1e-14)
    assert s.get_temperature(2) == pytest.approx(0.05 ** (2 / 3), rel=1e-14)
    assert s.get_temperature(3) == pytest.approx(0.05, rel=1e-14)
    s = VO.ExponentialTemperatureSchedule(3.0, 0.3, 11)
    assert s.get_temperature(5) == pytest.approx(3.0 * np.exp(np.log(0.1) * 0.5), rel=1e-14)


@pytest.mark.parametrize('cls', ['LinearTemperatureSchedule', 'ExponentialTemperatureSchedule'])
def test_schedule_quirks(VO, cls):
    S = getattr(VO, cls)
    s = S(1.0, 0.1, 5)
    with pytest.raises(RuntimeError):
        s.get_temperature(6)                       # it > num_steps
    s.get_temperature(5)                           # it == num_steps does not raise
    with pytest.raises(AssertionError):
        S(0.1, 1.0, 5)                             # T_final < T_init
    with pytest.raises(AssertionError):
        S(1.0, 1.0, 5)
    with pytest.raises(AssertionError):
        S(1.0, 0.1, 1)                             # num_steps > 1
    with pytest.raises(NotImplementedError):
        VO.TemperatureSchedule().get_temperature(0)


def test_temperature_state_forced_wins_and_missing_schedule_raises(VO):
    T = VO._EnergyTemperature()
    assert T.current == 1
    with pytest.raises(RuntimeError):
        T.update(0)                                # neither a schedule nor a forced value
    T.set_schedule('Exponential', T_init=1.0, T_final=0.05, num_steps=4)
    T.update(3)
    assert T.current == pytest.approx(0.05, rel=1e-14)
    T.forced = 0.7
    T.update(1)                                    # forced: the schedule is not evaluated
    assert T.current == 0.7 and T.value == pytest.approx(0.05, rel=1e-14)
    T.update(99)                                   # ... not even past its end
    T.forced = None
    T.set_linear_schedule(T_init=1, T_final=0.5, num_steps=3)
    T.update(1)
    assert T.current == pytest.approx(0.75, rel=1e-15)
    with pytest.raises(ValueError):
        T.set_linear_schedule()
    with pytest.raises(AssertionError):
        T.set_schedule('cosine', 1.0, 0.1, 4)
    with pytest.raises(AssertionError):
        T.set(-1.0)
    T.set(0.3)
    assert T.current == 0.3


# ---------------------------------------------------------------- host queries and argument checks
def test_vo_energy_form_host_query(lib):
    L = lib.lib()
    assert L.gpi_vo_energy_form(64, 8) == lib.VO_ENERGY_FUSED       # the bench grid
    assert L.gpi_vo_energy_form(128, 8) == lib.VO_ENERGY_TILED
    assert L.gpi_vo_energy_form(16, 32) == lib.VO_ENERGY_FUSED
    assert L.gpi_vo_energy_form(64, 32) == lib.VO_ENERGY_FUSED
    assert L.gpi_vo_energy_form(256, 32) == lib.VO_ENERGY_TILED
    assert L.gpi_vo_energy_form(1, 8) < 0
    assert L.gpi_vo_energy_form(64, 0) < 0
    assert L.gpi_vo_energy_form(64, 33) < 0
    assert L.gpi_vo_energy_workspace(128, 32, 8) > 32 * 2 * 128 * 128
    assert L.gpi_vo_energy_workspace(1, 32, 8) < 0


def test_vo_energy_argument_checks(lib):
    L = lib.lib()
    d = lib.VoEnergyDesc()                      # zeroed: missing buffers -> argument error, nothing launched
    assert L.gpi_vo_energy(C.byref(d), None) != 0
    assert L.gpi_vo_energy(None, None) != 0
    keep = [(C.c_double * 8)() for _ in range(6)]      # host memory standing in for the required buffers

    def desc(**kw):
        a = dict(n_fine=8, n=1, m_aux=4, n_iter=1, form=lib.VO_ENERGY_AUTO, temperature=1.0, length=0.1)
        a.update(kw)
        d = lib.VoEnergyDesc(**a)
        d.logkappa, d.bc, d.g, d.prec, d.mean, d.vars = [C.addressof(k) for k in keep]
        return d

    for bad in (dict(m_aux=33), dict(m_aux=0), dict(n_iter=4097), dict(n_iter=-1), dict(temperature=0.0),
                dict(temperature=-1.0), dict(temperature=float('nan')), dict(n_fine=1), dict(length=0.0),
                dict(form=7), dict(n=-1)):
        assert L.gpi_vo_energy(C.byref(desc(**bad)), None) == -1, bad
    for name in ('logkappa', 'bc', 'g', 'prec', 'mean', 'vars'):
        d = desc()
        setattr(d, name, None)
        assert L.gpi_vo_energy(C.byref(d), None) == -1, name
    # an explicit form that does not apply is unsupported, not an argument error; tiled needs its workspace
    assert L.gpi_vo_energy(C.byref(desc(n_fine=128, form=lib.VO_ENERGY_FUSED)), None) == -3
    assert L.gpi_vo_energy(C.byref(desc(form=lib.VO_ENERGY_TILED)), None) == -1
    assert L.gpi_vo_energy(C.byref(desc(n=0)), None) == 0          # empty batch: nothing to do


def test_energy_ensemble_refuses_foreign_samplers(VO):
    class Other(object):
        m = 4

    with pytest.raises(NotImplementedError, match='RadialBasisFunctionSampler'):
        VO.EnergyVirtualObservablesEnsemble([], 3, Other(), dtype=None, device=None)
