"""Time-modulated media (Medium.modulation_spec) on the emulator: the front end (parsing, validators, refusals, node lists), the five
scenarios of tests/modulation_case.py against the fp64 ModulatedOracle, the off reason, the handle's lifecycle, and a physics pin —
the mode amplitude of a uniformly modulated periodic box against the scheme's own scalar recurrence, off resonance (beating) and at
f_mod = 2 f_mode (parametric growth).  The device's pins are in tests/test_gpu_modulation.py."""
import dataclasses

import numpy as np
import pytest

import tidy3d_amd.schema as td
from tidy3d_amd import lib as L
from tidy3d_amd.constants import C_0
from tidy3d_amd.data import DataArray
from tidy3d_amd.discretize import discretize
from tidy3d_amd.engine import HipEngine
from tidy3d_amd.exceptions import SetupError, Tidy3dNotImplementedError

import list_case as lc
import modulation_case as mc
from cases import DL, PULSE


def _mod_dict(amplitude=0.5, phase=0.0):
    return {"type": "ModulationSpec", "conductivity": None,
            "permittivity": {"type": "SpaceTimeModulation",
                             "time_modulation": {"type": "ContinuousWaveTimeModulation", "freq0": 1e14, "amplitude": 0.5, "phase": 0.2},
                             "space_modulation": {"type": "SpaceModulation", "amplitude": amplitude, "phase": phase, "interp_method": "nearest"}}}


# ---------------------------------------------------------------------------------------------------------------- front end
def test_the_dict_form_parses():
    m = td.parse({"type": "Medium", "permittivity": 3.0, "conductivity": 0.0, "modulation_spec": _mod_dict()})
    assert isinstance(m, td.Medium) and isinstance(m.modulation_spec, td.ModulationSpec) and m.is_time_modulated
    stm = m.modulation_spec.permittivity
    assert isinstance(stm, td.SpaceTimeModulation) and isinstance(stm.time_modulation, td.ContinuousWaveTimeModulation)
    assert isinstance(stm.space_modulation, td.SpaceModulation) and m.modulation_spec.conductivity is None
    assert stm.time_modulation.freq0 == 1e14 and abs(stm.time_modulation.amp_complex - 0.5 * np.exp(0.2j)) < 1e-15
    assert abs(stm.max_modulation - 0.25) < 1e-15
    # the sign convention of the mirror's source-time classes: amplitude e^{i phase} e^{-i w t}
    t = 1.7e-15
    cwave = td.ContinuousWave(freq0=1e14, fwidth=1e13, amplitude=0.5, phase=0.2)
    assert abs(stm.time_modulation.amp_time(t) - 0.5 * np.exp(0.2j) * np.exp(-2j * np.pi * 1e14 * t)) < 1e-15
    assert abs(np.angle(stm.time_modulation.amp_time(t) / (cwave.amplitude * np.exp(1j * cwave.phase) * np.exp(-2j * np.pi * cwave.freq0 * t)))) < 1e-12
    # SpatialDataArray amplitude and phase (the dict form of a Python object carries the arrays themselves)
    coords = {"x": [-1.0, 1.0], "y": [0.0], "z": [0.0]}
    amp, ph = DataArray(np.array([0.2, 0.6]).reshape(2, 1, 1), coords), DataArray(np.array([0.0, 1.0]).reshape(2, 1, 1), coords)
    m2 = td.parse({"type": "Medium", "permittivity": 3.0, "modulation_spec": _mod_dict(amp, ph)})
    sp = m2.modulation_spec.permittivity.space_modulation
    assert abs(m2.modulation_spec.permittivity.max_modulation - 0.3) < 1e-15
    d = sp.sel_inside(np.array([-0.9, 0.9]), np.zeros(2), np.zeros(2))
    assert np.allclose(d, [0.2, 0.6 * np.exp(1j)])                     # nearest
    assert td.parse(m.dict()).modulation_spec.permittivity.time_modulation == stm.time_modulation
    # nonlinear_spec stays what it was
    assert isinstance(td.parse({"type": "Medium", "permittivity": 2.0, "nonlinear_spec": {"type": "NonlinearSpec"}}), td.Unsupported)


def test_validators_and_n_cfl():
    with pytest.raises(SetupError, match="permittivity"):
        mc.eps_modulated(eps=1.5, amp=0.6)
    assert mc.eps_modulated(eps=1.6, amp=0.6).is_time_modulated
    with pytest.raises(SetupError, match="conductivity"):
        mc.sigma_modulated(sigma=0.03, amp=0.04)
    stm = td.SpaceTimeModulation(time_modulation=mc.cw(amplitude=0.04))
    g = td.Medium(permittivity=2.0, conductivity=0.03, allow_gain=True, modulation_spec=td.ModulationSpec(conductivity=stm))
    assert g.is_time_modulated
    m = mc.eps_modulated(eps=4.0, amp=1.5)
    assert abs(m.n_cfl - np.sqrt(2.5)) < 1e-15 and abs(td.Medium(permittivity=4.0).n_cfl - 2.0) < 1e-15
    coords = {"x": [-1.0, 1.0], "y": [0.0], "z": [0.0]}
    sp = td.SpaceModulation(amplitude=DataArray(np.array([0.5, 2.0]).reshape(2, 1, 1), coords))
    assert abs(mc.eps_modulated(eps=4.0, amp=1.0, space=sp).n_cfl - np.sqrt(2.0)) < 1e-15
    # dt follows the lower bound: a medium of permittivity 1.44 - 0.44 = 1 does not shorten the step below vacuum's
    def dt_of(med):
        sim = mc._box_sim((8, 8, 8), td.BoundarySpec(x=mc._pec(), y=mc._pec(), z=mc._pec()),
                          [td.Structure(geometry=td.Box(center=(0, 0, 0), size=(0.2, 0.2, 0.2)), medium=med)])
        return discretize(sim, n_steps=1).spec.dt
    assert dt_of(mc.eps_modulated(eps=1.44, amp=0.44)) == dt_of(td.Medium(permittivity=1.0))


def _one_body(med, bspec=None, **kw):
    bspec = bspec or td.BoundarySpec(x=mc._pec(), y=mc._pec(), z=mc._pec())
    sim = mc._box_sim((12, 12, 12), bspec, [td.Structure(geometry=td.Box(center=(0, 0, 0), size=(0.3, 0.3, 0.3)), medium=med)])
    return dataclasses.replace(sim, **kw) if kw else sim


REFUSED_TYPES = {"PoleResidue": {"eps_inf": 2.0, "poles": []}, "Lorentz": {"eps_inf": 2.0, "coeffs": [[1.5, 4e14, 3e13]]},
                 "CustomMedium": {}, "AnisotropicMedium": {}, "FullyAnisotropicMedium": {}, "Medium2D": {}}


@pytest.mark.parametrize("tname", list(REFUSED_TYPES))
def test_media_other_than_medium_are_refused_on_use(tname):
    med = td.parse({"type": tname, **REFUSED_TYPES[tname], "modulation_spec": _mod_dict()})
    assert isinstance(med, td.Unsupported)                               # parsing never fails on it
    with pytest.raises(Tidy3dNotImplementedError, match=f"{tname} with 'modulation_spec'"):
        discretize(_one_body(med), n_steps=2)


def test_refusals_by_name(emu_lib):
    mod = mc.eps_modulated(eps=3.0, amp=0.5)
    with pytest.raises(Tidy3dNotImplementedError, match="modulation_spec.*component of 'AnisotropicMedium'"):
        discretize(_one_body(td.AnisotropicMedium(xx=mod, yy=td.Medium(permittivity=2.0), zz=td.Medium(permittivity=2.0))), n_steps=2)
    with pytest.raises(Tidy3dNotImplementedError, match="modulation_spec.*background"):
        discretize(_one_body(td.Medium(permittivity=2.0), medium=mod), n_steps=2)
    with pytest.raises(Tidy3dNotImplementedError, match="modulation_spec.*Simulation.symmetry"):
        discretize(_one_body(mod, symmetry=(1, 0, 0)), n_steps=2)
    absorber = td.BoundarySpec(x=mc._pec(), y=mc._pec(), z=td.Boundary.absorber(num_layers=6))
    slab = td.Structure(geometry=td.Box(center=(0, 0, 0), size=(0.2, 0.2, td.inf)), medium=mod)
    sim = _one_body(td.Medium(permittivity=2.0), bspec=absorber)
    with pytest.raises(Tidy3dNotImplementedError, match="modulation_spec.*Absorber"):
        discretize(dataclasses.replace(sim, structures=[slab]), n_steps=2)
    assert discretize(_one_body(mod, bspec=absorber), n_steps=2).spec.modulation          # clear of the layers: allowed
    eps = np.array([[2.5, 0.3, 0.0], [0.3, 2.2, 0.1], [0.0, 0.1, 2.0]])
    fa = td.Structure(geometry=td.Box(center=(0.2, 0.2, 0.2), size=(0.1, 0.1, 0.1)), medium=td.FullyAnisotropicMedium(permittivity=eps))
    sim = _one_body(mod)
    with pytest.raises(Tidy3dNotImplementedError, match="modulation_spec.*FullyAnisotropicMedium"):
        discretize(dataclasses.replace(sim, structures=list(sim.structures) + [fa]), n_steps=2)
    from tidy3d_amd import web
    with pytest.raises(Tidy3dNotImplementedError, match="modulation_spec.*more than one GPU"):
        web.run(_one_body(mod), devices=[0, 1], lib=emu_lib)
    spec = discretize(_one_body(mod), n_steps=2).spec
    with pytest.raises(Tidy3dNotImplementedError, match="modulation_spec.*z-slab"):
        HipEngine(spec, lib=emu_lib, force_comm=True)
    with pytest.raises(Tidy3dNotImplementedError, match="modulation_spec.*z-slab"):
        HipEngine(spec, lib=emu_lib, slab=(0, 6), rank=0, n_ranks=2)


def test_node_lists():
    spec = mc.scenario("pec_box_blocks").spec
    assert sorted(m.comp for m in spec.modulation) == [0, 0, 1, 1, 2, 2]
    for m in spec.modulation:
        assert m.d_eps.dtype == np.complex128 and m.d_sigma.dtype == np.complex128 and len(m.d_eps) == len(m.ijk) == len(m.d_sigma)
        if m.freq_eps:       # the permittivity block: amplitude 1, phase 0.3 folded in, uniform
            assert m.freq_sigma == 0.0 and np.allclose(m.d_eps, np.exp(0.3j)) and not m.d_sigma.any()
        else:
            assert m.freq_sigma == 0.7 * mc.F_MOD and np.allclose(m.d_sigma, 0.04 * np.exp(-0.4j)) and not m.d_eps.any()
        assert len(np.unique(m.ijk, axis=0)) == len(m.ijk)
    # a slab that reaches a PEC min wall: the wall-tangential nodes are not listed (the sweep holds them at zero)
    wall = discretize(mc._box_sim((8, 8, 8), td.BoundarySpec(x=mc._pec(), y=mc._pec(), z=mc._pec()),
                                  [td.Structure(geometry=td.Box(center=(0, 0, 0), size=(td.inf, td.inf, 0.2)), medium=mc.eps_modulated())]),
                      n_steps=1).spec
    for m in wall.modulation:
        for a in (0, 1):                      # (the slab is infinite along x and y)
            assert m.ijk[:, a].min() == (1 if a != m.comp else 0) and m.ijk[:, a].max() == 7


def test_zero_amplitude_is_the_plain_medium(emu_lib):
    zero = td.Medium(permittivity=3.0, conductivity=0.01, modulation_spec=td.ModulationSpec(
        permittivity=td.SpaceTimeModulation(time_modulation=mc.cw(amplitude=0.0)),
        conductivity=td.SpaceTimeModulation(time_modulation=mc.cw(), space_modulation=td.SpaceModulation(amplitude=0.0))))
    assert not zero.is_time_modulated
    a = discretize(_one_body(zero), n_steps=9).spec
    b = discretize(_one_body(td.Medium(permittivity=3.0, conductivity=0.01)), n_steps=9).spec
    assert a.modulation == [] and np.array_equal(a.mat_idx, b.mat_idx) and a.dt == b.dt
    out = []
    for spec in (a, b):
        with HipEngine(spec, lib=emu_lib) as e:
            e.run(9)
            out.append([e.get_field(c) for c in range(6)])
    assert all(np.array_equal(x, y) for x, y in zip(*out)) and np.abs(out[0][2]).max() > 0


# ---------------------------------------------------------------------------------------------------------------- scenarios
@pytest.mark.parametrize("label", list(mc.SCENARIOS))
def test_scenario_can_see_the_feature(label):
    sc = mc.scenario(label)
    for K in mc.KS:
        v = sc.visibility(K)
        print(f"[modulation] {label} K={K}: with / without the patch differ by {v:.3e} on the listed nodes")
        assert v >= 100 * mc.BAR, (label, K, v)


@pytest.mark.parametrize("K", mc.KS)
@pytest.mark.parametrize("label", mc.Scenario.all_labels())
def test_scenario_matches_the_modulated_oracle(label, K, emu_lib):
    mc.check_scenario(emu_lib, label, K)


def test_the_emulator_record_is_current(emu_lib):
    """tests/golden/modulation/emulator_k7.npz — what tests/test_gpu_modulation.py holds the device to — is this emulator's output, bit
    for bit (rewrite it with ``python tests/test_emu_modulation.py`` after a change that is meant to move it)"""
    want = np.load(mc.GOLDEN)
    got = mc.emulator_record(emu_lib)
    assert sorted(want.files) == sorted(got)
    for label in got:
        assert np.array_equal(got[label], want[label]), label


def test_off_reason(emu_lib):
    sim = mc._box_sim((128, 128, 64), td.BoundarySpec(x=mc._pec(), y=mc._pec(), z=mc._pec()),
                      [td.Structure(geometry=td.Box(center=(0, 0, 0), size=(0.4, 0.4, 0.4)), medium=mc.eps_modulated())])
    spec = discretize(sim, n_steps=4).spec
    spec.decay_every = 0
    lc.off_reason(emu_lib, spec, dataclasses.replace(spec, modulation=[]), 15, "time-modulated media")


# ---------------------------------------------------------------------------------------------------------------- lifecycle
def lifecycle(lib, variant=L.VARIANT_AUTO):
    """list_case.lifecycle on the PEC box, step pairs left on (the step count is part of the medium's state, nothing else is hidden
    in a PEC box)"""
    return lc.lifecycle(lib, mc.scenario("pec_box_blocks"), variant, twostep_off=False)


@pytest.mark.parametrize("variant", ["fused", "twopass"])
def test_lifecycle(variant, emu_lib):
    lifecycle(emu_lib, L.VARIANT_ZMARCH if variant == "twopass" else L.VARIANT_AUTO)


# ---------------------------------------------------------------------------------------------------------------- physics pin
N_Z, MODE, EPS_BAR, STEPS = 64, 4, 4.0, 200


def pin_spec(f_mod, depth, phase):
    per = td.Boundary.periodic()
    med = mc.eps_modulated(eps=EPS_BAR, amp=depth * EPS_BAR, freq0=f_mod, phase=phase)
    sim = mc._box_sim((4, 4, N_Z), td.BoundarySpec(x=per, y=per, z=per),
                      [td.Structure(geometry=td.Box(center=(0, 0, 0), size=(td.inf, td.inf, td.inf)), medium=med)], sources=())
    spec = discretize(dataclasses.replace(sim, subpixel=False), n_steps=STEPS).spec
    spec.decay_every = 0
    assert spec.shape == (4, 4, N_Z) and sum(len(m.ijk) for m in spec.modulation) == 3 * 16 * N_Z
    return spec


def mode_shape(spec):
    zb = np.asarray(spec.boundaries[2])[:-1]
    return np.cos(2.0 * np.pi * MODE * (zb - zb[0]) / (N_Z * DL))


def recurrence(spec, f_mod, depth, phase, a0):
    """D_{n+1} - 2 D_n + D_{n-1} = -(c dt k~)^2 D_n / eps(n dt), E_n = D_n / eps(n dt); H^{-1/2} = 0: D_1 - D_0 = -(c dt k~)^2 E_0"""
    k = 2.0 * np.pi * MODE / (N_Z * DL)
    q = (C_0 * spec.dt * (2.0 / DL) * np.sin(0.5 * k * DL)) ** 2
    eps = lambda n: EPS_BAR + np.real(depth * EPS_BAR * np.exp(1j * phase) * np.exp(-2j * np.pi * f_mod * n * spec.dt))      # noqa: E731
    D = np.zeros(STEPS + 1)
    D[0] = a0 * eps(0)
    D[1] = D[0] - q * a0
    for n in range(1, STEPS):
        D[n + 1] = 2.0 * D[n] - D[n - 1] - q * D[n] / eps(n)
    return D / np.array([eps(n) for n in range(STEPS + 1)])


def amplitudes(stepper, spec, a0):
    """the amplitude of the mode in E_x after every step, from an object with set / step / get"""
    shape = mode_shape(spec)
    ex0 = np.broadcast_to((a0 * shape)[:, None, None], (N_Z, 4, 4))
    out = [a0]
    stepper.start(ex0)
    for _ in range(STEPS):
        ex = stepper.step()
        out.append(float(2.0 * np.mean(ex * shape[:, None, None])))
        resid = ex - out[-1] * shape[:, None, None]
        assert np.abs(resid).max() <= 1e-4 * max(abs(a0), np.abs(ex).max())         # it stays one mode
    return np.array(out)


class _OracleStepper:
    def __init__(self, spec):
        self.o = mc.ModulatedOracle(spec)

    def start(self, ex0):
        self.o.E[0][...] = ex0

    def step(self):
        self.o.step()
        return np.array(self.o.E[0])


class _EngineStepper:
    def __init__(self, engine):
        self.e = engine

    def start(self, ex0):
        self.e.set_field(0, ex0.astype(np.float32))

    def step(self):
        self.e.run(1)
        return self.e.get_field(0).astype(np.float64)


def f_mode(spec):
    k = 2.0 * np.pi * MODE / (N_Z * DL)
    return np.arcsin(C_0 * spec.dt / np.sqrt(EPS_BAR) * np.sin(0.5 * k * DL) / DL) / (np.pi * spec.dt)


@pytest.mark.parametrize("case", ["beating", "growth"])
def test_mode_amplitude_follows_the_recurrence(case, emu_lib):
    # (a standing wave started at its E maximum: the modulation's phase decides whether it starts in the growing or in the decaying
    #  quadrature of the parametric resonance — -pi / 2 is the growing one)
    depth, phase, a0 = 0.2, -0.5 * np.pi, 1e-3
    f0 = f_mode(pin_spec(1e14, depth, phase))                 # (dt depends on the lower bound of the permittivity, not on f_mod)
    f_mod = 2.0 * f0 if case == "growth" else 2.9 * f0
    spec = pin_spec(f_mod, depth, phase)
    want = recurrence(spec, f_mod, depth, phase, a0)
    ref = amplitudes(_OracleStepper(spec), spec, a0)
    assert np.abs(ref - want).max() <= 1e-10 * np.abs(want).max(), np.abs(ref - want).max() / np.abs(want).max()
    with HipEngine(spec, lib=emu_lib) as e:
        got = amplitudes(_EngineStepper(e), spec, np.float64(np.float32(a0)))
    want32 = recurrence(spec, f_mod, depth, phase, np.float64(np.float32(a0)))
    err = np.abs(got - want32).max() / np.abs(want32).max()
    peak_last = np.abs(want[-40:]).max()
    print(f"[modulation] {case}: f_mode {f0:.4e} Hz, f_mod {f_mod:.4e} Hz, engine vs recurrence {err:.3e} of the largest amplitude, "
          f"largest |a| over the last 40 steps / a0 = {peak_last / a0:.3f}")
    assert err <= mc.BAR
    if case == "growth":
        assert peak_last >= 2.0 * a0
    else:
        env = np.abs(want)
        assert env.max() < 1.6 * a0 and peak_last < 1.6 * a0                # bounded: beating, not growth


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "hipemu"))
    import build_emu
    from tidy3d_amd.lib import load_library
    os.makedirs(os.path.dirname(mc.GOLDEN), exist_ok=True)
    np.savez_compressed(mc.GOLDEN, **mc.emulator_record(load_library(build_emu.build())))
    print("wrote", mc.GOLDEN, os.path.getsize(mc.GOLDEN), "bytes")
