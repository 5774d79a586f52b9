"""The flux of a DirectivityMonitor reduced on the device from its lattice accumulators (``fdtd_lattice_flux``,
csrc/fdtd_lattice_flux.hpp), on the CPU emulator: against the host formula on the downloaded accumulators on every surface and
frequency, with a bar that is derived, not measured; partial waves, partial workgroups and the stride loop; the excluded surface;
split runs, fdtd_reset, the engine's axis renaming; web.run on both paths; the library's refusals.  Scenes: tests/directivity_case.py."""
import ctypes
import dataclasses

import numpy as np
import pytest

import tidy3d_amd.schema as td
from tidy3d_amd import lib as L
from tidy3d_amd import web
from tidy3d_amd.discretize import discretize
from tidy3d_amd.engine import HipEngine

import directivity_case as case
import projection_dft_case as pcase


def test_the_entry_points_are_there(emu_lib):
    for name in ("fdtd_set_lattice_flux_weights", "fdtd_lattice_flux"):
        assert hasattr(emu_lib.dll, name) and name in L.SYMBOLS


def check_kernel_a(lib, repeat):
    sim = case.scene_a()
    only = dataclasses.replace(sim, monitors=[sim.monitors[0]])
    worst = case.check_kernel(only, lib, case.N_STEPS, case.A_NODES, repeat=repeat)
    print(f"[directivity] scene A: worst |device - host formula| / bar = {worst:.3e}")


def test_kernel_scene_a(emu_lib):
    """13 x 13 = 169 points per face: two full waves, a partial one and an idle one (the repeat after fdtd_reset: scenes B and C
    here, every scene on the device)"""
    check_kernel_a(emu_lib, repeat=False)


@pytest.mark.parametrize("scene", ["b", "c"])
def test_kernel_scenes_b_and_c(emu_lib, scene):
    """600 points (two rounds of the stride loop and a partial third), 75 and 72 (a partial second wave, odd and even), 63 (a single
    partial wave); z- excluded; the split run and the repeat after fdtd_reset give the same bits"""
    sim, nodes = (case.scene_b(), case.B_NODES) if scene == "b" else (case.scene_c(), case.C_NODES)
    worst = case.check_kernel(sim, emu_lib, case.B_STEPS, nodes)
    print(f"[directivity] scene {scene.upper()}: worst |device - host formula| / bar = {worst:.3e}")


@pytest.mark.parametrize("shift", [1, 2])
def test_renamed_axes(emu_lib, shift):
    """the engine's cyclic axis renaming: the normal and the weight vectors are renamed with the axes, the result is the same"""
    got = {}
    for s in (0, shift):
        k = case.Kernel(case.scene_c(), emu_lib, case.B_STEPS, axis_shift=s)
        try:
            k.engine.run(case.B_STEPS)
            got[s] = (k.engine.lattice_flux(), k.host_flux(k.engine.results()))
        finally:
            k.close()
    for n, (flux, bar) in got[0][1].items():
        assert np.all(np.abs(got[shift][0][n] - flux) <= bar), (n, got[shift][0][n], flux, bar)
        assert np.all(np.abs(got[shift][0][n] - got[0][0][n]) <= bar), n


def end_to_end(lib, sim, steps, runs=None):
    """web.run with the flux on the device against the host path: flux and directivity within the bar the far fields of the two
    paths are held to (tests/projection_dft_case.py END_BAR), of the largest value per frequency"""
    a, b = runs or [web.run(sim, n_steps=steps, lib=lib, verbose=False, projection_device=dev, return_tidy3d=False) for dev in (True, False)]
    assert "Flux of DirectivityMonitor 'dir': device" in a.log and "Flux of DirectivityMonitor 'dir': host" in b.log
    assert "Projection monitor accumulated on its lattice on the device: " in a.log and "on its lattice" not in b.log
    da, db = a["dir"], b["dir"]
    fa, fb = np.asarray(da.flux.values), np.asarray(db.flux.values)
    Da, Db = np.asarray(da.directivity.values), np.asarray(db.directivity.values)
    r_flux = np.abs(fa - fb) / np.abs(fb)
    r_dir = np.abs(Da - Db).max(axis=(0, 1, 2)) / np.abs(Db).max(axis=(0, 1, 2))
    print(f"[directivity] device against host path: flux {r_flux / pcase.EPS32} x 2^-24, directivity {r_dir / pcase.EPS32} x 2^-24 "
          f"(bar {pcase.END_BAR / pcase.EPS32:g} x 2^-24)")
    assert fa.dtype == fb.dtype == np.float64 and (r_flux <= pcase.END_BAR).all() and (r_dir <= pcase.END_BAR).all(), (r_flux, r_dir)


def test_web_run_on_both_paths(emu_lib):
    """the tiny scene (y+ excluded, a custom origin) through web.run: the log names the path, the results agree"""
    end_to_end(emu_lib, case.tiny_scene(), case.TINY_STEPS)


def library_refusals(lib):
    """fdtd_lattice_flux and fdtd_set_lattice_flux_weights refuse, with the handle's error string: an id that is no lattice monitor
    (a whole-box DFT monitor; an id out of range), a lattice monitor without weights, weights that do not fit, z-slab handles, the
    handles of a Bloch pair"""
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)             # noqa: E731
    out = np.full(2, np.nan)
    sim = case.tiny_scene()
    mon = sim.monitors[0]
    flux = td.FluxMonitor(center=mon.center, size=(0, 0.2, 0.2), freqs=case.FREQS, name="plane")
    ang = td.parse(dict(mon.dict(), type="FieldProjectionAngleMonitor", name="ang"))
    spec = discretize(dataclasses.replace(sim, monitors=[flux, ang, mon]), n_steps=8, projection_device=True).spec
    assert [m.kind for m in spec.monitors] == ["dft"] + ["dft_lattice"] * 10
    with HipEngine(spec, lib=lib, axis_shift=0) as e:
        e.run(4)
        d, h = e.lib.dll, e.handle
        for bad, msg in ((0, "no lattice accumulators"), (11, "bad id"), (-1, "bad id"), (1, "no integration weights")):
            assert d.fdtd_lattice_flux(h, bad, p(out)) < 0 and msg in e.lib.error(h) and "fdtd_lattice_flux" in e.lib.error(h), (bad, e.lib.error(h))
            assert np.isnan(out).all()
        n3, w = np.asarray([3, 3, 3], dtype=np.int32), np.ones(64)
        assert d.fdtd_set_lattice_flux_weights(h, 0, 0, 1.0, p(n3), p(w), p(w), p(w)) < 0 and "no lattice accumulators" in e.lib.error(h)
        assert d.fdtd_set_lattice_flux_weights(h, 1, 0, 1.0, p(n3), p(w), p(w), p(w)) < 0 and "weights along axis" in e.lib.error(h)
        assert d.fdtd_set_lattice_flux_weights(h, 3, 0, 1.0, p(n3), p(w), p(w), p(w)) < 0 and "does not hold component 1" in e.lib.error(h)
        assert d.fdtd_set_lattice_flux_weights(h, 6, 0, 1.0, p(n3), p(w), p(w), p(w)) < 0 and "has its weights already" in e.lib.error(h)
        assert d.fdtd_lattice_flux(h, 6, p(out)) == 0 and np.isfinite(out).all()
        assert set(e.lattice_flux()) == {f"dir::{s}" for s in ("x-", "x+", "y-", "z-", "z+")}
    per = td.BoundarySpec(x=td.Boundary.pml(num_layers=4), y=td.Boundary.pml(num_layers=4), z=td.Boundary.periodic())
    pspec = discretize(dataclasses.replace(sim, boundary_spec=per, monitors=[]), n_steps=8).spec
    with HipEngine(pspec, lib=lib, force_comm=True) as e:          # (one rank exchanging with itself around the periodic z axis)
        assert e.lib.dll.fdtd_lattice_flux(e.handle, 0, p(out)) < 0 and "z-slab" in e.lib.error(e.handle)
    bloch = td.BoundarySpec(x=td.Boundary.pml(num_layers=4), y=td.Boundary.pml(num_layers=4), z=td.Boundary.bloch(0.3))
    bspec = discretize(dataclasses.replace(sim, boundary_spec=bloch, monitors=[]), n_steps=8).spec
    with HipEngine(bspec, lib=lib) as e:
        e.run(2)
        for hh in (e.handle, e.twin.handle):
            assert e.lib.dll.fdtd_lattice_flux(hh, 0, p(out)) < 0 and "Bloch pair" in e.lib.error(hh)


def test_library_refusals(emu_lib):
    library_refusals(emu_lib)
