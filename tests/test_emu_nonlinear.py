"""Kerr media (Medium.nonlinear_spec with NonlinearSusceptibility models) on the emulator: the entry points (``schema.with_nonlinear``,
the mirror object, refusals by name), the node lists, the five scenarios of tests/nonlinear_case.py against the fp64 NonlinearOracle,
the iteration count, chi3 = 0, the Jacobi order, the axis renamings, the off reason, the handle's lifecycle, and a physics pin — the
phase a travelling plane wave accumulates against the Yee-grid dispersion relation at eps_eff = eps + (3/4) chi3 A^2.  The device's
pins are in tests/test_gpu_nonlinear.py."""
import dataclasses
import json

import numpy as np
import pytest

import tidy3d_amd.schema as td
from tidy3d_amd import lib as L
from tidy3d_amd.constants import C_0, MU_0
from tidy3d_amd.discretize import discretize
from tidy3d_amd.engine import HipEngine, permute_spec
from tidy3d_amd.exceptions import Tidy3dNotImplementedError

import dense_state as ds
import list_case as lc
import modulation_case as mc
import nonlinear_case as nc
from cases import DL


def _spec_dict(chi3=(1e-3,), num_iters=5):
    return {"type": "NonlinearSpec", "num_iters": num_iters,
            "models": [{"type": "NonlinearSusceptibility", "chi3": c, "numiters": 7} for c in chi3]}


def _medium_dict(nonlinear_spec, tname="Medium", **kw):
    return {"type": tname, "permittivity": 3.0, "conductivity": 0.0, **kw, "nonlinear_spec": nonlinear_spec}


def _one_body(med, bspec=None, **kw):
    bspec = bspec or nc._PEC3()
    sim = mc._box_sim((12, 12, 12), bspec, [nc._bx((0, 0, 0), (0.3, 0.3, 0.3), med)], sources=(nc.DIPOLE,))
    return dataclasses.replace(sim, **kw) if kw else sim


def _fields(spec, lib, steps=5, **kw):
    with HipEngine(spec, lib=lib, **kw) as e:
        e.run(steps)
        return [e.get_field(c) for c in range(6)]


# ---------------------------------------------------------------------------------------------------------------- entry points
def test_parse_keeps_the_placeholder_and_with_nonlinear_resolves_it():
    raw = _medium_dict(_spec_dict((1e-3, 5e-4)))
    u = td.parse(raw)
    assert isinstance(u, td.Unsupported) and u.type == "Medium with 'nonlinear_spec'"
    with pytest.raises(Tidy3dNotImplementedError, match="Medium with 'nonlinear_spec'"):
        u.fail()
    sim = td.with_nonlinear(_one_body(u))
    med = sim.structures[0].medium
    assert isinstance(med, td.Medium) and isinstance(med.nonlinear_spec, td.NonlinearSpec) and med.is_nonlinear
    assert med.permittivity == 3.0 and med.nonlinear_spec.num_iters == 5 and abs(med.nonlinear_spec.chi3 - 1.5e-3) < 1e-18      # several models sum
    assert all(isinstance(m, td.NonlinearSusceptibility) for m in med.nonlinear_spec.models)
    assert med.n_cfl == td.Medium(permittivity=3.0).n_cfl
    assert td.with_nonlinear(sim) is sim                                   # nothing left to resolve: the same object
    d = med.dict()                                                         # written back, and still a placeholder for parse
    assert d["nonlinear_spec"]["type"] == "NonlinearSpec" and d["nonlinear_spec"]["models"][0]["chi3"] == 1e-3
    assert isinstance(td.parse(d), td.Unsupported)
    assert td.with_nonlinear(_one_body(td.parse(d))).structures[0].medium == med
    assert "nonlinear_spec" in td.Medium(permittivity=2.0).dict() and not td.Medium(permittivity=2.0).is_nonlinear
    # the reference's older form: the model itself in place of the spec
    old = td.with_nonlinear(_one_body(td.parse(_medium_dict({"type": "NonlinearSusceptibility", "chi3": 2e-3})))).structures[0].medium
    assert old.is_nonlinear and old.nonlinear_spec.chi3 == 2e-3


REFUSED_SPECS = {
    "TwoPhotonAbsorption": {"type": "NonlinearSpec", "models": [{"type": "TwoPhotonAbsorption", "beta": 1e-3}], "num_iters": 5},
    "KerrNonlinearity": {"type": "NonlinearSpec", "models": [{"type": "KerrNonlinearity", "n2": 1e-3}], "num_iters": 5},
    "complex chi3": {"type": "NonlinearSpec", "models": [{"type": "NonlinearSusceptibility", "chi3": {"real": 1e-3, "imag": 1e-4}}]},
    "without models": {"type": "NonlinearSpec", "models": [], "num_iters": 5},
}


@pytest.mark.parametrize("what", list(REFUSED_SPECS))
def test_other_models_stay_placeholders_that_name_the_model(what):
    sim = td.with_nonlinear(_one_body(td.parse(_medium_dict(REFUSED_SPECS[what]))))
    assert isinstance(sim.structures[0].medium, td.Unsupported)
    with pytest.raises(Tidy3dNotImplementedError, match=f"Medium with 'nonlinear_spec'.*{what}"):
        discretize(sim, n_steps=2)


@pytest.mark.parametrize("tname", ["PoleResidue", "Lorentz", "CustomMedium", "AnisotropicMedium", "Medium2D"])
def test_media_other_than_medium_are_refused_on_use(tname):
    extra = {"PoleResidue": {"eps_inf": 2.0, "poles": []}, "Lorentz": {"eps_inf": 2.0, "coeffs": [[1.5, 4e14, 3e13]]}}.get(tname, {})
    raw = {"type": tname, **extra, "nonlinear_spec": _spec_dict()}
    med = td.parse(raw)
    assert isinstance(med, td.Unsupported)
    with pytest.raises(Tidy3dNotImplementedError, match=f"{tname} with 'nonlinear_spec'"):
        discretize(_one_body(med), n_steps=2)


def test_refusals_by_name(emu_lib):
    kerr = nc.kerr(eps=3.0, chi3=1e-3)
    with pytest.raises(Tidy3dNotImplementedError, match="nonlinear_spec.*component of 'AnisotropicMedium'"):
        discretize(_one_body(td.AnisotropicMedium(xx=kerr, yy=td.Medium(permittivity=2.0), zz=td.Medium(permittivity=2.0))), n_steps=2)
    with pytest.raises(Tidy3dNotImplementedError, match="nonlinear_spec.*background"):
        discretize(_one_body(td.Medium(permittivity=2.0), medium=kerr), n_steps=2)
    with pytest.raises(Tidy3dNotImplementedError, match="nonlinear_spec.*Simulation.symmetry"):
        discretize(_one_body(kerr, symmetry=(1, 0, 0)), n_steps=2)
    bloch = td.Boundary(minus=td.BlochBoundary(bloch_vec=0.1), plus=td.BlochBoundary(bloch_vec=0.1))
    with pytest.raises(Tidy3dNotImplementedError, match="nonlinear_spec.*Bloch"):
        discretize(_one_body(kerr, bspec=td.BoundarySpec(x=bloch, y=mc._pec(), z=mc._pec())), n_steps=2)
    absorber = td.BoundarySpec(x=mc._pec(), y=mc._pec(), z=td.Boundary.absorber(num_layers=6))
    slab = nc._bx((0, 0, 0), (0.2, 0.2, td.inf), kerr)
    with pytest.raises(Tidy3dNotImplementedError, match="nonlinear_spec.*Absorber"):
        discretize(dataclasses.replace(_one_body(kerr, bspec=absorber), structures=[slab]), n_steps=2)
    assert discretize(_one_body(kerr, bspec=absorber), n_steps=2).spec.nonlinear           # clear of the layers: allowed
    sim = _one_body(kerr)
    sheet = td.Structure(geometry=td.Box(center=(0, 0, 0), size=(0.2, 0.2, 0)), medium=td.Medium2D(ss=td.Medium(conductivity=0.01), tt=td.Medium(conductivity=0.01)))
    with pytest.raises(Tidy3dNotImplementedError, match="Medium2D sheet inside a nonlinear"):
        discretize(dataclasses.replace(sim, structures=list(sim.structures) + [sheet]), n_steps=2)
    eps = np.array([[2.5, 0.3, 0.0], [0.3, 2.2, 0.1], [0.0, 0.1, 2.0]])
    fa = nc._bx((0.2, 0.2, 0.2), (0.1, 0.1, 0.1), td.FullyAnisotropicMedium(permittivity=eps))
    with pytest.raises(Tidy3dNotImplementedError, match="nonlinear_spec.*FullyAnisotropicMedium"):
        discretize(dataclasses.replace(sim, structures=list(sim.structures) + [fa]), n_steps=2)
    mod = nc._bx((0.2, 0.2, 0.2), (0.1, 0.1, 0.1), mc.eps_modulated(eps=3.0, amp=0.5))
    with pytest.raises(Tidy3dNotImplementedError, match="nonlinear_spec.*modulation_spec"):
        discretize(dataclasses.replace(sim, structures=list(sim.structures) + [mod]), n_steps=2)
    pec = nc._bx((0.2, 0.2, 0.2), (0.1, 0.1, 0.1), td.PEC)
    conformal = dataclasses.replace(sim, structures=list(sim.structures) + [pec], subpixel=td.SubpixelSpec(pec=td.PECConformal()))
    with pytest.raises(Tidy3dNotImplementedError, match="nonlinear_spec.*PECConformal"):
        discretize(conformal, n_steps=2)
    from tidy3d_amd import web
    with pytest.raises(Tidy3dNotImplementedError, match="nonlinear_spec.*more than one GPU"):
        web.run(sim, devices=[0, 1], lib=emu_lib)
    spec = discretize(sim, n_steps=2).spec
    with pytest.raises(Tidy3dNotImplementedError, match="nonlinear_spec.*z-slab"):
        HipEngine(spec, lib=emu_lib, force_comm=True)
    with pytest.raises(Tidy3dNotImplementedError, match="nonlinear_spec.*z-slab"):
        HipEngine(spec, lib=emu_lib, slab=(0, 6), rank=0, n_ranks=2)


def test_dict_mirror_and_reference_objects_give_equal_fields(emu_lib, tmp_path):
    from tidy3d_amd import web
    mirror = _one_body(td.Medium(permittivity=3.0, nonlinear_spec=td.NonlinearSpec(models=(td.NonlinearSusceptibility(chi3=1e-3),
                                                                                            td.NonlinearSusceptibility(chi3=5e-4)))))
    mon = td.FieldTimeMonitor(center=(0, 0, 0), size=(0.2, 0.2, 0.2), name="ft", interval=1, fields=("Ex", "Ez"))
    mirror = dataclasses.replace(mirror, monitors=[mon])
    as_dict = json.loads(json.dumps(mirror.dict()))
    assert as_dict["structures"][0]["medium"]["nonlinear_spec"]["models"][1]["chi3"] == 5e-4
    fname = tmp_path / "sim.json"
    fname.write_text(json.dumps(as_dict))
    runs = {"mirror": web.run(mirror, n_steps=6, lib=emu_lib, verbose=False), "dict": web.run(as_dict, n_steps=6, lib=emu_lib, verbose=False),
            "json": web.run(str(fname), n_steps=6, lib=emu_lib, verbose=False)}
    try:
        import tidy3d
        runs["tidy3d"] = web.run(tidy3d.Simulation.parse_obj(as_dict), n_steps=6, lib=emu_lib, verbose=False, return_tidy3d=False)
    except ImportError:
        pass
    want = np.asarray(runs["mirror"]["ft"].Ez.values)
    assert np.abs(want).max() > 0
    for k, r in runs.items():
        for f in ("Ex", "Ez"):
            assert np.array_equal(np.asarray(getattr(r["ft"], f).values), np.asarray(getattr(runs["mirror"]["ft"], f).values)), (k, f)
    n_nodes = sum(len(s.ijk) for s in discretize(mirror, n_steps=6).spec.nonlinear)
    assert any(f"Nonlinear (Kerr) media: {n_nodes} nodes listed, 5 fixed-point iterations per step; single time steps." in ln
               for ln in str(runs["dict"].log).splitlines())


def test_node_lists():
    sc = nc.scenario("pec_box_blocks")
    assert sorted(s.comp for s in sc.spec.nonlinear) == [0, 1, 2]                   # one set per component, merged over the media
    for s in sc.spec.nonlinear:
        assert len(np.unique(s.ijk, axis=0)) == len(s.ijk) == len(s.chi3) and s.nbr_ijk.shape == (len(s.ijk), 8, 3)
        a = s.comp
        assert s.nbr_comp == ((a + 1) % 3,) * 4 + ((a + 2) % 3,) * 4 and s.num_iters == 5
    # a slab that reaches a PEC min wall: the wall-tangential nodes are not listed; slots beyond a wall are empty
    wall = discretize(mc._box_sim((8, 8, 8), nc._PEC3(), [nc._bx((0, 0, 0), (td.inf, td.inf, 0.2), nc.kerr())]), n_steps=1).spec
    for s in wall.nonlinear:
        for a in (0, 1):
            assert s.ijk[:, a].min() == (1 if a != s.comp else 0) and s.ijk[:, a].max() == 7
        assert (s.nbr_ijk[:, :, 0] < 0).any() == (s.comp != 2)         # (E_x at i = 7 reaches for E_y, E_z at i = 8; E_z stays inside)
    with pytest.raises(Tidy3dNotImplementedError, match="different num_iters"):
        discretize(mc._box_sim((8, 8, 8), nc._PEC3(), [nc._bx((-0.1, 0, 0), (0.1, 0.2, 0.2), nc.kerr(num_iters=3)),
                                                       nc._bx((0.1, 0, 0), (0.1, 0.2, 0.2), nc.kerr(eps=2.0))]), n_steps=1)


# ---------------------------------------------------------------------------------------------------------------- scenarios
@pytest.mark.parametrize("label", list(nc.SCENARIOS))
def test_scenario_can_see_the_feature(label):
    sc = nc.scenario(label)
    for K in (0,) + nc.KS:
        s = sc.strength(K)
        print(f"[nonlinear] {label} K={K}: max |chi3| I / eps_bar over the listed nodes {s:.3f}")
        assert nc.RANGE[0] <= s <= nc.RANGE[1], (label, K, s)
    for K in nc.KS:
        v = sc.visibility(K)
        print(f"[nonlinear] {label} K={K}: with / without the lists differ by {v:.3e} on the listed nodes")
        assert v >= 100 * nc.BAR, (label, K, v)


def test_iterations_are_counted():
    sc = nc.scenario("pec_box_blocks")
    for K in nc.KS:
        d = sc.listed_diff(sc.ref(K, 5), sc.ref(K, 1))
        print(f"[nonlinear] pec_box_blocks K={K}: num_iters 1 against 5 differ by {d:.3e} on the listed nodes")
        assert d > 10 * nc.BAR, (K, d)


@pytest.mark.parametrize("num_iters", nc.ITERS)
@pytest.mark.parametrize("K", nc.KS)
@pytest.mark.parametrize("label", nc.Scenario.all_labels())
def test_scenario_matches_the_nonlinear_oracle(label, K, num_iters, emu_lib):
    nc.check_scenario(emu_lib, label, K, num_iters)


@pytest.mark.parametrize("label", list(nc.SCENARIOS))
def test_chi3_zero_gives_the_bits_of_the_plain_spec(label, emu_lib):
    sc = nc.scenario(label)
    for path in nc.PATHS:
        zero = sc.run(emu_lib, 7, path, scale=0.0)
        plain = sc.run(emu_lib, 7, path, plain=True)
        for c in range(6):
            assert np.array_equal(zero.fields[c], plain.fields[c]), (label, path, ds.COMP[c])


def test_jacobi_order(emu_lib):
    sc = nc.scenario("pec_box_blocks")
    a, b = sc.run(emu_lib, 7, "fused"), sc.run(emu_lib, 7, "fused", reverse=True)
    for c in range(6):
        assert np.array_equal(a.fields[c], b.fields[c]), ds.COMP[c]


@pytest.mark.parametrize("shift", [1, 2])
def test_axis_renamings(shift, emu_lib):
    """``permute_spec`` renames the lists: the renamed problem gives the fields of the user's, under the bar"""
    sc = nc.scenario("graded_two_media")
    p = permute_spec(sc.spec, shift)
    for s, t in zip(sc.spec.nonlinear, p.nonlinear):
        assert t.comp == (s.comp - shift) % 3 and t.nbr_comp == ((t.comp + 1) % 3,) * 4 + ((t.comp + 2) % 3,) * 4
    got = ds.run_engine(sc.spec, emu_lib, sc.state, 7, "fused", axis_shift=shift)
    assert max(sc.errors(got.fields, 7)) <= nc.BAR
    sc.check_nodes(got.fields, 7, f"fused shift {shift}")
    for K in nc.KS[:-1]:                                     # node by node at the other step counts as well
        sc.check_nodes(ds.run_engine(sc.spec, emu_lib, sc.state, K, "fused", axis_shift=shift).fields, K, f"fused shift {shift}")


def test_the_emulator_record_is_current(emu_lib):
    """tests/golden/nonlinear/emulator_k7.npz — what tests/test_gpu_nonlinear.py holds the device to — is this emulator's output, bit
    for bit (rewrite it with ``python tests/test_emu_nonlinear.py`` after a change that is meant to move it)"""
    want = np.load(nc.GOLDEN)
    got = nc.emulator_record(emu_lib)
    assert sorted(want.files) == sorted(got)
    for label in got:
        assert np.array_equal(got[label], want[label]), label


def off_reason(lib):
    sim = mc._box_sim((128, 128, 64), nc._PEC3(), [nc._bx((0, 0, 0), (0.4, 0.4, 0.4), nc.kerr(chi3=1e-3))], sources=(nc.DIPOLE,))
    spec = discretize(sim, n_steps=4).spec
    spec.decay_every = 0
    lc.off_reason(lib, spec, dataclasses.replace(spec, nonlinear=[]), 17, "nonlinear (Kerr) media")


def test_off_reason(emu_lib):
    off_reason(emu_lib)


# ---------------------------------------------------------------------------------------------------------------- lifecycle
def lifecycle(lib, variant=L.VARIANT_AUTO):
    """list_case.lifecycle, and a list added to a live handle between runs against a fresh handle that reached the same step count and
    was given that state (I^n is formed from the fields in front of every step, nothing is carried).  The graded PEC box: no CPML
    and no dispersive body, whose states a set_field would not replace."""
    sc = nc.scenario("graded_two_media")

    def late_list(engine, load, fields, whole):
        """three steps with two components' lists, then the third's, against a fresh handle from that state"""
        with engine(dataclasses.replace(sc.spec, nonlinear=[s for s in sc.spec.nonlinear if s.comp != 2])) as e:
            load(e)
            e.run(3)
            at3 = fields(e)
            e.add_nonlinear([s for s in sc.spec.nonlinear if s.comp == 2])
            e.run(4)
            late = fields(e)
        with engine() as e:
            load(e)
            e.run(3)                 # (the step count is part of the state: the dipole's waveform follows it)
            load(e, at3)
            e.run(4)
            late_fresh = fields(e)
        for c in range(6):
            assert np.array_equal(late[c], late_fresh[c]) and not np.array_equal(late[c], whole[c]), ds.COMP[c]
    return lc.lifecycle(lib, sc, variant, steps=late_list)


@pytest.mark.parametrize("variant", ["fused", "twopass"])
def test_lifecycle(variant, emu_lib):
    lifecycle(emu_lib, L.VARIANT_ZMARCH if variant == "twopass" else L.VARIANT_AUTO)


# ---------------------------------------------------------------------------------------------------------------- physics pin
N_Z, MODE, EPS, RATIO, PERIODS = 96, 8, 4.0, 0.02, 40
# what the fp64 NonlinearOracle's accumulated phase deviates by from the Yee-grid dispersion relation at eps_eff = eps + (3/4) chi3 A^2
# (recorded from this test, docs/history/NONLINEAR.md); the test's bar is twice that
ORACLE_DEVIATION = 4.915e-2          # rad, of a Kerr phase shift of 1.879 rad over 40.0 periods (1710 steps): 2.6 %
PIN_BAR = None if ORACLE_DEVIATION is None else 2.0 * ORACLE_DEVIATION


def pin_spec(chi3_a2_over_eps, amp, steps=1):
    per = td.Boundary.periodic()
    med = nc.kerr(eps=EPS, chi3=chi3_a2_over_eps * EPS / amp ** 2)
    sim = mc._box_sim((4, 4, N_Z), td.BoundarySpec(x=per, y=per, z=per), [nc._bx((0, 0, 0), (td.inf, td.inf, td.inf), med)], sources=())
    spec = discretize(dataclasses.replace(sim, subpixel=False), n_steps=steps).spec
    spec.decay_every = 0
    assert spec.shape == (4, 4, N_Z) and sum(len(s.ijk) for s in spec.nonlinear) == 3 * 16 * N_Z
    return spec


def yee_omega_dt(spec, eps):
    """w dt of the Yee grid for the wave vector of the pin: sin(w dt / 2) = c dt / (sqrt(eps) dz) sin(k dz / 2)"""
    k = 2.0 * np.pi * MODE / (N_Z * DL)
    return 2.0 * np.arcsin(C_0 * spec.dt / (np.sqrt(eps) * DL) * np.sin(0.5 * k * DL))


def travelling_wave(spec, amp, eps):
    """E_x^0 = A cos(k z), H_y^{-1/2} of the wave that travels along +z in the linear medium ``eps`` on the Yee grid"""
    zb = np.asarray(spec.boundaries[2])[:-1]
    k = 2.0 * np.pi * MODE / (N_Z * DL)
    wdt = yee_omega_dt(spec, eps)
    h0 = amp * spec.dt / (MU_0 * DL) * np.sin(0.5 * k * DL) / np.sin(0.5 * wdt)
    ex = amp * np.cos(k * (zb - zb[0]))
    hy = h0 * np.cos(k * (zb - zb[0] + 0.5 * DL) + 0.5 * wdt)
    shape = (N_Z, 4, 4)
    return np.broadcast_to(ex[:, None, None], shape).copy(), np.broadcast_to(hy[:, None, None], shape).copy()


def phase_of(spec, ex):
    """phi of E_x = a cos(k z - phi), from the projection on the fundamental"""
    zb = np.asarray(spec.boundaries[2])[:-1]
    k = 2.0 * np.pi * MODE / (N_Z * DL)
    line = np.asarray(ex, np.float64).mean(axis=(1, 2))
    return float(np.arctan2(np.sum(line * np.sin(k * (zb - zb[0]))), np.sum(line * np.cos(k * (zb - zb[0])))))


def _wrap(x):
    return float((x + np.pi) % (2.0 * np.pi) - np.pi)


def pin_measure(lib=None):
    """-> dict of the figures of the physics pin (the engine's only with ``lib``)"""
    amp = 1e-3
    spec = pin_spec(RATIO, amp)
    eps_eff = EPS * (1.0 + 0.75 * RATIO)
    steps = int(round(PERIODS * 2.0 * np.pi / yee_omega_dt(spec, eps_eff)))
    ex0, hy0 = travelling_wave(spec, amp, eps_eff)
    out = {"steps": steps, "phase_eff": steps * yee_omega_dt(spec, eps_eff), "phase_lin": steps * yee_omega_dt(spec, EPS)}

    def run_oracle(sp):
        o = nc.NonlinearOracle(sp)
        o.E[0][...] = ex0
        o.H[1][...] = hy0
        for _ in range(steps):
            o.step()
        return [np.array(f) for f in o.E + o.H]
    ref = run_oracle(spec)
    lin = run_oracle(dataclasses.replace(spec, nonlinear=[]))
    out["oracle_deviation"] = abs(_wrap(phase_of(spec, ref[0]) - out["phase_eff"]))
    out["linear_miss"] = abs(_wrap(phase_of(spec, lin[0]) - out["phase_eff"]))
    if lib is not None:
        with HipEngine(spec, lib=lib) as e:
            e.set_field(0, ex0.astype(np.float32))
            e.set_field(4, hy0.astype(np.float32))
            e.run(steps)
            got = [e.get_field(c) for c in range(6)]
        out["engine_deviation"] = abs(_wrap(phase_of(spec, got[0]) - out["phase_eff"]))
        out["engine_vs_oracle"] = max(float(np.linalg.norm(got[c] - ref[c]) / np.linalg.norm(ref[c])) for c in (0, 4))
    return out


def test_plane_wave_phase_follows_the_effective_permittivity(emu_lib):
    m = pin_measure(emu_lib)
    print("[nonlinear] physics pin: " + ", ".join(f"{k} {v:.4e}" if isinstance(v, float) else f"{k} {v}" for k, v in m.items()))
    assert PIN_BAR is not None, "record ORACLE_DEVIATION from the printed figures"
    assert m["oracle_deviation"] <= PIN_BAR
    assert m["engine_vs_oracle"] <= nc.BAR
    assert m["engine_deviation"] <= PIN_BAR
    assert m["linear_miss"] >= 5.0 * PIN_BAR


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "hipemu"))
    import build_emu
    from tidy3d_amd.lib import load_library
    os.makedirs(os.path.dirname(nc.GOLDEN), exist_ok=True)
    np.savez_compressed(nc.GOLDEN, **nc.emulator_record(load_library(build_emu.build())))
    print("wrote", nc.GOLDEN, os.path.getsize(nc.GOLDEN), "bytes")
