"""PEC-conformal boundaries (SubpixelSpec.pec = PECConformal) on the CPU: the operator tests (stability of the clamped scheme, the
resonances of a circular cavity against the staircase), the front end (selection, dict form, refusals), and on the emulator the
scenarios of tests/pec_conformal_case.py against the fp64 ConformalOracle, the off reason, the handle's lifecycle and the record the
device is held to.  The device's pins are in tests/test_gpu_pec_conformal.py.

Measured (docs/history/PEC_CONFORMAL.md): mean relative error of (TM010, TE11) over 8 centre offsets — staircase 4.362e-2, 7.737e-2 at
a = 8 cells and 2.234e-2, 4.053e-2 at a = 16; conformal 1.055e-2, 1.811e-2 and 5.169e-3, 8.753e-3: ratios 4.13, 4.27, 4.32, 4.63; the
test's factor is half the smallest, 2.067.  The conformal errors fall at order 1.03 (TM010) and 1.05 (TE11): the area clamp, which
the stability test needs, touches every triangular face and keeps the scheme at first order with a four times smaller constant."""
import dataclasses

import numpy as np
import pytest

import tidy3d_amd.schema as td
from tidy3d_amd import lib as L
from tidy3d_amd.discretize import discretize
from tidy3d_amd.engine import HipEngine
from tidy3d_amd.exceptions import Tidy3dNotImplementedError

import list_case as lc
import pec_conformal_case as pc
from cases import DL, PULSE

FACTOR = 2.067           # half the smallest measured staircase / conformal ratio (4.135), no lower than 2
OFFSETS = np.random.default_rng(11).uniform(-0.5, 0.5, size=(12, 3))
CAVITY_OFFSETS = np.random.default_rng(12).uniform(-0.5, 0.5, size=(8, 2))


# ---------------------------------------------------------------------------------------------------------------- operators
def test_the_clamped_scheme_is_stable_and_the_unclamped_one_is_not():
    worst_on, worst_off = 0.0, 0.0
    specs = [lambda clamp, o=o: pc.sphere_in_box(o, clamp=clamp) for o in OFFSETS]
    specs += [lambda clamp, a=a: pc.cylinder_in_box(a, OFFSETS[a], clamp=clamp) for a in range(3)]
    for n, make in enumerate(specs):
        lam = pc.largest_eigenvalue(make(None))
        print(f"[pec-conformal] operator {n}: largest eigenvalue of W_e W_h {lam:.4f}")
        worst_on = max(worst_on, lam)
        assert lam < 4.0, (n, lam)
    for make in (specs[0], specs[4], specs[12]):
        worst_off = max(worst_off, pc.largest_eigenvalue(make(0.0)))
    print(f"[pec-conformal] largest eigenvalue: clamped {worst_on:.4f}, clamp off {worst_off:.2f}")
    assert worst_off > 4.0              # without the clamp the same bodies break the leapfrog limit: the test does see the clamp


def test_cavity_resonances_converge_and_beat_the_staircase():
    mean = {}
    for a in (8, 16):
        for name, sub in (("staircase", pc.STAIRCASE), ("conformal", pc.CONFORMAL)):
            mean[(a, name)] = np.mean([pc.cavity_errors(a, o, sub) for o in CAVITY_OFFSETS], axis=0)
            print(f"[pec-conformal] cavity a = {a} cells {name}: mean relative error TM010 {mean[(a, name)][0]:.3e} TE11 {mean[(a, name)][1]:.3e}")
    for m in range(2):
        order = np.log2(mean[(8, "conformal")][m] / mean[(16, "conformal")][m])
        print(f"[pec-conformal] mode {('TM010', 'TE11')[m]}: conformal convergence order {order:.2f}")
        assert mean[(16, "conformal")][m] < mean[(8, "conformal")][m]
        for a in (8, 16):
            assert FACTOR * mean[(a, "conformal")][m] <= mean[(a, "staircase")][m], (a, m, mean[(a, "conformal")][m], mean[(a, "staircase")][m])


# ---------------------------------------------------------------------------------------------------------------- front end
def _sphere_sim(subpixel, bspec=pc.PEC_WALLS, N=(12, 12, 12), **kw):
    body = td.Structure(geometry=td.Sphere(center=(0.013, 0.021, -0.008), radius=3.6 * DL), medium=td.PEC)
    sim = pc._box_sim(N, bspec, [body], sources=[td.PointDipole(center=(-0.25, 0.0, 0.0), source_time=PULSE, polarization="Ez")], subpixel=subpixel)
    return dataclasses.replace(sim, **kw) if kw else sim


def test_selection_and_the_dict_form():
    p = td.parse({"type": "PECConformal", "attrs": {}, "timestep_reduction": 0.3})
    assert isinstance(p, td.PECConformal) and p == td.PECConformal() and abs(p.courant_ratio - 0.7) < 1e-15
    parsed = td.parse({"type": "SubpixelSpec", "attrs": {}, "dielectric": {"type": "PolarizedAveraging"}, "metal": {"type": "Staircasing"},
                       "pec": {"type": "PECConformal", "timestep_reduction": 0.25}})
    mirror = td.SubpixelSpec(pec=td.PECConformal(timestep_reduction=0.25))
    assert parsed.courant_ratio(True) == mirror.courant_ratio(True) == 0.75 and parsed.courant_ratio(False) == 1.0
    a, b = discretize(_sphere_sim(parsed), n_steps=2).spec, discretize(_sphere_sim(mirror), n_steps=2).spec
    assert a.dt == b.dt and np.array_equal(a.mat_idx, b.mat_idx) and len(a.conformal) == len(b.conformal) == 3
    for x, y in zip(a.conformal, b.conformal):
        assert np.array_equal(x.ijk, y.ijk) and np.array_equal(x.d, y.d) and np.array_equal(x.nbr_ijk, y.nbr_ijk)
    # everything else keeps the staircase: True (at the reduced step it always had), False, SubpixelSpec(), Staircasing, the heuristic
    stair = discretize(_sphere_sim(pc.STAIRCASE), n_steps=2).spec
    for sub in (True, False, td.SubpixelSpec(), td.SubpixelSpec(pec=td.parse({"type": "HeuristicPECStaircasing"}))):
        s = discretize(_sphere_sim(sub), n_steps=2).spec
        assert not s.conformal and np.array_equal(s.mat_idx == 0, stair.mat_idx == 0), sub
    t = discretize(_sphere_sim(True), n_steps=2).spec
    assert abs(t.dt / stair.dt - 0.7) < 1e-12 and a.dt / stair.dt == pytest.approx(0.75)
    # no PEC medium: no lists, the full step
    free = dataclasses.replace(_sphere_sim(pc.CONFORMAL), structures=[])
    assert not discretize(free, n_steps=2).spec.conformal


def test_lists_and_raster():
    spec = pc.scenario("sphere_blocks").spec
    stair = discretize(dataclasses.replace(discretize_sim("sphere_blocks"), subpixel=pc.STAIRCASE), n_steps=2).spec
    assert sorted(cs.comp for cs in spec.conformal) == [3, 4, 5]
    changed = spec.mat_idx != stair.mat_idx
    assert changed.any() and ((stair.mat_idx == 0) & (spec.mat_idx > 1)).any()          # edges freed into the blocks' media
    for cs in spec.conformal:
        assert cs.d.dtype == np.float32 and cs.d.shape == (len(cs.ijk), 4) and len(np.unique(cs.ijk, axis=0)) == len(cs.ijk)
        assert (cs.area >= 0).all() and (cs.area <= 1).all() and (cs.l >= 0).all() and (cs.l <= 1).all()
        assert np.allclose(cs.area_eff, np.maximum(cs.area, 0.49 * cs.l.max(axis=1)))
        assert (cs.l.max(axis=1) / cs.area_eff <= 1.0 / 0.49 + 1e-12).all()
        for k in range(4):                # an edge is PEC iff l == 0, and then the slot is empty
            j = cs.nbr_ijk[:, k]
            ok = j[:, 0] >= 0
            assert (spec.mat_idx[cs.nbr_comp[k]][j[ok, 2], j[ok, 1], j[ok, 0]] != 0).all() and (cs.l[ok, k] > 0).all()
            assert not cs.d[~ok, k].any()
    # the area of the sphere's equatorial cut, summed from the face fractions of Hz on one plane, against pi r^2
    body = td.Structure(geometry=td.Sphere(center=(0.011, -0.017, 0.5 * DL), radius=6.3 * DL), medium=td.PEC)
    s = pc._spec(pc._box_sim((20, 20, 4), pc.PEC_WALLS, [body]))
    cz = next(cs for cs in s.conformal if cs.comp == 5)
    on = cz.ijk[:, 2] == 2                                  # the faces of Hz lie on the plane z = zb[2] = 0: 0.5 DL below the centre
    full_pec = ((s.mat_idx[0][2] == 0) & (np.roll(s.mat_idx[0][2], -1, axis=0) == 0) & (s.mat_idx[1][2] == 0) & (np.roll(s.mat_idx[1][2], -1, axis=1) == 0)).sum()
    pec_area = (full_pec + float(np.sum(1.0 - cz.area[on]))) * DL * DL
    want = np.pi * ((6.3 * DL) ** 2 - (0.5 * DL) ** 2)
    assert abs(pec_area / want - 1.0) < 5e-3, (pec_area, want)


def discretize_sim(label):
    """the Simulation behind scenario ``label`` (rebuilt: the scenarios keep their specs only)"""
    assert label == "sphere_blocks"
    bodies = [td.Structure(geometry=td.Box(center=(-0.35, 0.05, 0.1), size=(0.3, 0.4, 0.5)), medium=td.Medium(permittivity=3.0)),
              td.Structure(geometry=td.Box(center=(0.3, -0.1, -0.2), size=(0.3, 0.4, 0.5)), medium=td.Lorentz(eps_inf=2.0, coeffs=[(1.5, 4e14, 3e13)])),
              td.Structure(geometry=td.Sphere(center=(0.043, -0.031, 0.067), radius=6.3 * DL), medium=td.PEC)]
    return pc._box_sim((24, 20, 28), pc.PEC_WALLS, bodies)


def test_refusals_by_name(emu_lib):
    with pytest.raises(Tidy3dNotImplementedError, match="PECConformal.*Simulation.symmetry"):
        discretize(_sphere_sim(pc.CONFORMAL, symmetry=(1, 0, 0)), n_steps=2)
    pmc_plus = td.BoundarySpec(x=td.Boundary(minus=td.PECBoundary(), plus=td.PMCBoundary()), y=pc._pec(), z=pc._pec())
    with pytest.raises(Tidy3dNotImplementedError, match="PECConformal.*PMC boundary on a plus face"):
        discretize(_sphere_sim(pc.CONFORMAL, bspec=pmc_plus), n_steps=2)
    bloch = td.BoundarySpec(x=td.Boundary(minus=td.BlochBoundary(bloch_vec=0.1), plus=td.BlochBoundary(bloch_vec=0.1)), y=pc._pec(), z=pc._pec())
    with pytest.raises(Tidy3dNotImplementedError, match="PECConformal.*Bloch"):
        discretize(_sphere_sim(pc.CONFORMAL, bspec=bloch), n_steps=2)
    sim = _sphere_sim(pc.CONFORMAL)
    eps = np.array([[2.5, 0.3, 0.0], [0.3, 2.2, 0.1], [0.0, 0.1, 2.0]])
    fa = td.Structure(geometry=td.Box(center=(0.2, 0.2, 0.2), size=(0.1, 0.1, 0.1)), medium=td.FullyAnisotropicMedium(permittivity=eps))
    with pytest.raises(Tidy3dNotImplementedError, match="PECConformal.*FullyAnisotropicMedium"):
        discretize(dataclasses.replace(sim, structures=list(sim.structures) + [fa]), n_steps=2)
    import modulation_case as mc
    mod = td.Structure(geometry=td.Box(center=(0.2, 0.2, 0.2), size=(0.1, 0.1, 0.1)), medium=mc.eps_modulated())
    with pytest.raises(Tidy3dNotImplementedError, match="PECConformal.*modulation_spec"):
        discretize(dataclasses.replace(sim, structures=list(sim.structures) + [mod]), n_steps=2)
    from tidy3d_amd import web
    with pytest.raises(Tidy3dNotImplementedError, match="PECConformal.*more than one GPU"):
        web.run(sim, devices=[0, 1], lib=emu_lib)
    spec = discretize(sim, n_steps=2).spec
    with pytest.raises(Tidy3dNotImplementedError, match="PECConformal.*z-slab"):
        HipEngine(spec, lib=emu_lib, force_comm=True)
    with pytest.raises(Tidy3dNotImplementedError, match="PECConformal.*z-slab"):
        HipEngine(spec, lib=emu_lib, slab=(0, 6), rank=0, n_ranks=2)
    # a PMC min wall is covered
    pmc_min = td.BoundarySpec(x=td.Boundary(minus=td.PMCBoundary(), plus=td.PECBoundary()), y=pc._pec(), z=pc._pec())
    assert discretize(_sphere_sim(pc.CONFORMAL, bspec=pmc_min), n_steps=2).spec.conformal


# ---------------------------------------------------------------------------------------------------------------- engine
@pytest.mark.parametrize("label", list(pc.SCENARIOS))
def test_scenario_can_see_the_correction(label):
    v = pc.scenario(label).visibility(1)
    print(f"[pec-conformal] {label}: fp64 oracle without the correction differs by {v:.3e} over the listed H nodes after 1 step")
    assert v >= pc.VISIBLE


@pytest.mark.parametrize("K", pc.KS)
@pytest.mark.parametrize("run_label", list(pc.RUNS))
def test_scenario_matches_the_conformal_oracle(run_label, K, emu_lib):
    pc.check_run(emu_lib, run_label, K, what="emulator ")


def test_the_committed_record_is_the_emulators(emu_lib):
    rec = pc.emulator_record(emu_lib)       # (the file is written from this dict: np.savez_compressed(pc.GOLDEN, **rec))
    want = np.load(pc.GOLDEN)
    assert sorted(want.files) == sorted(rec)
    for label, v in rec.items():
        assert v.dtype == np.float32 and np.array_equal(v.view(np.uint32), want[label].view(np.uint32)), label


def off_reason(lib):
    """128 x 128 x 64, 4 steps: no pairs under reason 16; the same grid staircased takes pairs"""
    body = td.Structure(geometry=td.Sphere(center=(0.013, 0.021, -0.008), radius=10.3 * DL), medium=td.PEC)
    spec, stair = (pc._spec(pc._box_sim((128, 128, 64), pc.PEC_WALLS, [body], subpixel=sub), n_steps=4) for sub in (pc.CONFORMAL, pc.STAIRCASE))
    assert spec.conformal and not stair.conformal
    lc.off_reason(lib, spec, stair, 16, "PEC-conformal boundaries")


def lifecycle(lib, variant):
    """list_case.lifecycle without the set_field in mid-run (the Lorentz block's pole states); fdtd_reset keeps the lists"""
    sc = pc.scenario("sphere_blocks")

    def against_plain(engine, load, fields, whole):
        with engine(sc.plain) as e:
            load(e)
            e.run(7)
            plain = fields(e)
        assert any(not np.array_equal(whole[c], plain[c]) for c in range(3, 6))      # the lists were there, also after the reset
    lc.lifecycle(lib, sc, variant, mid=False, steps=against_plain, axis_shift=0)


def test_off_reason(emu_lib):
    off_reason(emu_lib)


@pytest.mark.parametrize("variant", ["fused", "twopass"])
def test_lifecycle(variant, emu_lib):
    lifecycle(emu_lib, L.VARIANT_ZMARCH if variant == "twopass" else L.VARIANT_AUTO)


def test_web_run_returns_data_and_logs_the_faces(emu_lib):
    from tidy3d_amd import web
    sim = _sphere_sim(pc.CONFORMAL)
    mon = td.FieldTimeMonitor(center=(0, 0, 0), size=(td.inf, td.inf, 0), name="ft", interval=4)
    data = web.run(dataclasses.replace(sim, monitors=[mon]), n_steps=24, lib=emu_lib, verbose=False)
    n = sum(len(cs.ijk) for cs in discretize(sim, n_steps=24).spec.conformal)
    assert f"{n} cut faces listed" in data.log and n > 0
    assert np.isfinite(np.asarray(data["ft"].Ez.values)).all() and np.abs(np.asarray(data["ft"].Ez.values)).max() > 0
