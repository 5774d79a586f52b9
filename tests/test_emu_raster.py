"""Box, Sphere and Cylinder structures rasterised on the device (``fdtd_rasterize``, ``raster_paint_kernel``, csrc/fdtd_raster.hpp;
``rasterize_device=True``) on the CPU emulator, held to the host path of ``discretize.rasterize`` — equal uint16 indices, equal
material tables: faces on grid lines, infinite extents, bodies outside the domain, the order of overwrites, surfaces through nodes,
per-component media, two x tiles; the whole-call fallbacks and their log line; the rest of set-up (sub-pixel averaging, PEC-conformal
lists, web.run) behind it; the engine's axis renamings; the interface's refusals.  Scenes: tests/raster_case.py."""
import ctypes
import dataclasses

import numpy as np
import pytest

import tidy3d_amd.schema as td
from tidy3d_amd import lib as L
from tidy3d_amd import web
from tidy3d_amd.discretize import discretize
from tidy3d_amd.engine import permute_spec
from tidy3d_amd.exceptions import SetupError

import raster_case as case


def test_the_entry_point_is_there(emu_lib):
    assert hasattr(emu_lib.dll, "fdtd_rasterize") and "fdtd_rasterize" in L.SYMBOLS
    assert ctypes.sizeof(L.FdtdRasterRecord) == 4 * (2 + 3 + 9 + 9 + 1) + 8 * 6 and ctypes.sizeof(L.FdtdRasterJob) == 4 * 6 + 8 + 8 * 9 + 8


def boxes(lib):
    """scene 1 in both orders: 37 nodes along x are neither a multiple of the 64-node tile nor of a row of four"""
    assert case.nodes_on_faces(case.scene_boxes()) > 0
    fwd, host_fwd = case.check_scene(lib, "boxes", case.scene_boxes(), shape=(37, 21, 13))
    rev, host_rev = case.check_scene(lib, "boxes_rev", case.scene_boxes(reverse=True), shape=(37, 21, 13))
    assert not np.array_equal(host_fwd.mat_idx, host_rev.mat_idx)              # the order of the structures matters ...
    assert {m.eps_inf for m in fwd.media[1:]} == {m.eps_inf for m in rev.media[1:]}      # ... for the nodes, not for the media
    assert (fwd.mat_idx == 0).any()                                            # the PEC box
    found = {fwd.media[i].eps_inf for i in np.unique(fwd.mat_idx) if i}
    assert {5.0, 6.0, 8.0} <= found and 7.0 not in found                       # on grid lines, infinite, one node thick; not the outside one
    six = next(i for i, m in enumerate(fwd.media) if i and m.eps_inf == 6.0)
    assert (fwd.mat_idx[2] == six).any(axis=(1, 2)).all()                      # the infinite box reaches every plane along z
    eight = next(i for i, m in enumerate(fwd.media) if i and m.eps_inf == 8.0)
    assert len(np.unique(np.argwhere(fwd.mat_idx[1] == eight)[:, 2])) == 1     # one node thick along x


def test_boxes(emu_lib):
    boxes(emu_lib)


def test_autogrid_snapped_faces(emu_lib):
    sim = case.scene_autogrid()
    dev, _ = case.check_scene(emu_lib, "autogrid", sim)
    geo = sim.structures[0].geometry
    for a in range(3):                      # the mesher put grid lines on both faces of the box
        for face in (geo.center[a] - geo.size[a] / 2, geo.center[a] + geo.size[a] / 2):
            assert np.isclose(np.asarray(dev.boundaries[a]), face, rtol=0, atol=1e-12).any(), (a, face)


def spheres(lib):
    dev, _ = case.check_scene(lib, "spheres", case.scene_spheres(), shape=(24, 20, 16), launches=3)
    # centred on an Ez node: the Ez nodes on the axes and at the 3-4-5 triples lie on the surface exactly, and are inside
    xs, ys, zs = (np.asarray(v, float) for v in dev.yee_coords(2))
    c = case.scene_spheres().structures[0].geometry.center
    d2 = (xs[None, None, :] - c[0]) ** 2 + (ys[None, :, None] - c[1]) ** 2 + (zs[:, None, None] - c[2]) ** 2
    on = d2 == (5 * case.DL) ** 2
    assert on.sum() >= 6 + 24 and (dev.mat_idx[2][on] == 2).all() and (dev.mat_idx[2][d2 > (5 * case.DL) ** 2] == 1).all()
    case.check_scene(lib, "spheres_graded", case.scene_spheres_graded(), shape=(37, 21, 13))


def test_spheres(emu_lib):
    spheres(emu_lib)


def cylinders(lib):
    dev, _ = case.check_scene(lib, "cylinders", case.scene_cylinders(), shape=(37, 21, 13))
    per_comp = [set(np.unique(dev.mat_idx[c])) for c in range(3)]
    assert per_comp[0] != per_comp[1] != per_comp[2]                            # the diagonal medium: one index per component
    assert any(m.poles for m in dev.media)                                     # the dispersive one
    return dev


def test_cylinders(emu_lib):
    cylinders(emu_lib)


def test_two_x_tiles(emu_lib):
    dev, _ = case.check_scene(emu_lib, "tiles", case.scene_two_tiles(), shape=(264, 8, 12))
    assert (dev.mat_idx[:, :, :, 255] != 1).any() and (dev.mat_idx[:, :, :, 256] != 1).any()


@pytest.mark.parametrize("kind", ["polyslab", "medium2d", "kerr"])
def test_fallback(emu_lib, kind):
    """one structure outside the device rasteriser: the whole call takes the host path and the log says which structure"""
    sim, words = case.fallback_scenes()[kind]
    host = case.host_spec("fallback_" + kind, sim)
    dev = discretize(sim, n_steps=4, rasterize_device=True, lib=emu_lib).spec
    case.same_raster(dev, host)
    first, last = dev.raster_log.splitlines()
    assert first.startswith("rasterize_device: " + words) and first.endswith("the whole call takes the host path.")
    assert last == "Rasterised 9 structures: host." == host.raster_log


def set_up(lib):
    """behind ``rasterize``: sub-pixel averaging of the sphere scene and the PEC-conformal lists of the box scene read the device
    path's array as they read the host's"""
    sub = dataclasses.replace(case.scene_spheres_graded(), subpixel=True)
    dev, host = case.check_scene(lib, "subpixel", sub)
    assert len(dev.media) > 5                                                   # (averaged entries exist)
    conf = dataclasses.replace(case.scene_boxes(), subpixel=td.SubpixelSpec(pec=td.PECConformal()))
    dev, host = case.check_scene(lib, "conformal", conf)
    assert dev.conformal and len(dev.conformal) == len(host.conformal)
    for a, b in zip(dev.conformal, host.conformal):
        for f in dataclasses.fields(a):
            va, vb = getattr(a, f.name), getattr(b, f.name)
            assert np.array_equal(va, vb) if isinstance(va, np.ndarray) else va == vb, f.name


def test_rest_of_set_up(emu_lib):
    set_up(emu_lib)


def run_both(lib):
    """40 steps of the sphere scene with a FieldMonitor: the two paths give the same bits, the log names the path"""
    sim = dataclasses.replace(case.scene_spheres_graded(), monitors=[
        td.FieldMonitor(center=(0, 0, 0), size=(0.6, 0.5, 0), freqs=[3e14], name="f")])
    a, b = [web.run(sim, n_steps=40, lib=lib, verbose=False, return_tidy3d=False, rasterize_device=dev) for dev in (True, False)]
    assert "Rasterised 3 structures: device (9 launches)." in a.log.splitlines()
    assert "Rasterised 3 structures: host." in b.log.splitlines()
    for f in ("Ex", "Ey", "Ez", "Hx", "Hy", "Hz"):
        va, vb = np.asarray(getattr(a["f"], f).values), np.asarray(getattr(b["f"], f).values)
        assert np.abs(vb).max() > 0 and np.array_equal(va, vb), f


def test_web_run_on_both_paths(emu_lib):
    run_both(emu_lib)


@pytest.mark.parametrize("shift", [0, 1, 2])
def test_renamed_axes(emu_lib, shift):
    dev, host = case.check_scene(emu_lib, "cylinders", case.scene_cylinders())
    pa, pb = permute_spec(dev, shift), permute_spec(host, shift)
    assert np.array_equal(pa.mat_idx, pb.mat_idx) and pa.shape == pb.shape and pa.media == pb.media


def test_symmetric_and_pmc_plus_grids(emu_lib):
    """the recursive discretisations (Simulation.symmetry, PMC on a plus face) pass the keyword on"""
    sym = dataclasses.replace(case.scene_spheres(), symmetry=(1, 0, 0), sources=[
        td.PointDipole(center=(0.0, 0.1, 0.0), source_time=case.PULSE, polarization="Ex")])
    dev, _ = case.check_scene(emu_lib, "symmetry", sym)
    assert "device" in dev.raster_log
    walls = td.BoundarySpec(x=td.Boundary(minus=td.PECBoundary(), plus=td.PMCBoundary()), y=td.Boundary.pec(), z=td.Boundary.pec())
    dev, _ = case.check_scene(emu_lib, "pmc_plus", dataclasses.replace(case.scene_spheres(), boundary_spec=walls))
    assert "device" in dev.raster_log and dev.mirror_plus[0] > 0


def job_of(lib, n=1, kind=L.RASTER_BOX, hi=4):
    rec = L.FdtdRasterRecord(kind=kind)
    for c in range(3):
        rec.medium[c] = 2
        for a in range(3):
            rec.hi[c][a] = hi
            rec.size[a] = 1.0
    recs = (L.FdtdRasterRecord * 1)(rec)
    xs = np.linspace(0.0, 1.0, 4)
    job = L.FdtdRasterJob(struct_bytes=ctypes.sizeof(L.FdtdRasterJob), record_bytes=ctypes.sizeof(L.FdtdRasterRecord), device=0,
                          nx=4, ny=4, nz=4, n=n, records=recs)
    for q in range(9):
        job.coords[q] = xs.ctypes.data
    return job, (recs, xs)


def interface_refusals(lib):
    """fdtd_rasterize refuses, each with its words and before any launch (the output stays as it was): a null pointer, n == 0, an
    unknown kind, an index box outside the shape, a layout of another header; rasterize_device=True without a library"""
    out = np.full((3, 4, 4, 4), 7, np.uint16)
    p = out.ctypes.data_as(ctypes.c_void_p)
    call = lambda job, o=p: lib.dll.fdtd_rasterize(ctypes.byref(job) if job is not None else None, o)       # noqa: E731
    job, keep = job_of(lib)
    assert call(job) == 0 and (out == 2).any() and (out[:, 0, 0, 0] == 2).all()         # (the job itself is fine)
    out[...] = 7
    cases = [(None, p, "null argument"), (job, None, "null argument")]
    for bad, o, words in cases:
        assert call(bad, o) < 0 and words in lib.error(None)
    job, keep = job_of(lib)
    job.coords[4] = None
    assert call(job) < 0 and "null argument" in lib.error(None)
    job, keep = job_of(lib)
    job.records = None
    assert call(job) < 0 and "null argument" in lib.error(None)
    job, keep = job_of(lib, n=0)
    assert call(job) < 0 and "no records (n == 0)" in lib.error(None)
    job, keep = job_of(lib, kind=3)
    assert call(job) < 0 and "unknown kind 3" in lib.error(None)
    job, keep = job_of(lib, hi=5)
    assert call(job) < 0 and "outside the shape" in lib.error(None)
    job, keep = job_of(lib)
    job.records[0].lo[1][2] = -1
    assert call(job) < 0 and "outside the shape" in lib.error(None)
    job, keep = job_of(lib)
    job.struct_bytes += 8
    assert call(job) < 0 and "this library has" in lib.error(None)
    assert (out == 7).all()
    for c in range(3):
        assert "fdtd_rasterize" in lib.error(None)


def test_interface_refusals(emu_lib):
    interface_refusals(emu_lib)


def test_device_path_without_a_library(monkeypatch, tmp_path):
    monkeypatch.setenv("TIDY3D_AMD_LIBRARY", str(tmp_path / "libfdtd_hip.so"))
    with pytest.raises(SetupError, match="rasterize_device=True needs the HIP solver library"):
        discretize(case.scene_boxes(), n_steps=4, rasterize_device=True)
    assert discretize(case.scene_boxes(), n_steps=4, rasterize_device=False).spec.raster_log.endswith("host.")


def test_unset_keyword_is_the_host_path():
    import tidy3d_amd.discretize as D
    assert D.RASTER_DEVICE_CELLS is None
    assert discretize(case.scene_two_tiles(), n_steps=4).spec.raster_log == "Rasterised 2 structures: host."
