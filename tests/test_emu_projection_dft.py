"""Projection-monitor surfaces accumulated on their sampling lattice only, on the device (MonitorSpec kind "dft_lattice",
csrc/fdtd_lattice_dft.hpp), on the CPU emulator: against the host path of the same engine and against the fp64 oracle, the projected
fields and the files of web.run on both paths, bit for bit across schedules, the engine's axis renaming, fdtd_reset, monitors added
to a live handle and reads in mid-run; the device memory the library reports; the choice between the two paths and its refusals.
The case, the bars and the figures measured: tests/projection_dft_case.py."""
import ctypes
import dataclasses
import json

import numpy as np
import pytest

import tidy3d_amd.schema as td
from tidy3d_amd import discretize as D
from tidy3d_amd import lib as L
from tidy3d_amd.discretize import discretize
from tidy3d_amd.engine import HipEngine
from tidy3d_amd.exceptions import DataError, SolverLibraryError, Tidy3dNotImplementedError

import projection_dft_case as case

N_SURF = 10         # six of `box`, one each of the four planes


@pytest.fixture(scope="module")
def ctx(emu_lib):
    """the two discretizations, run A (device path, fused single steps) and run B (host path), computed once"""
    dd, dh = case.discs()
    raw_a, _ = case.run_engine(dd.spec, emu_lib)
    raw_b, _ = case.run_engine(dh.spec, emu_lib)
    return dict(dd=dd, dh=dh, raw_a=raw_a, raw_b=raw_b)


def test_the_feature_is_there(ctx, emu_lib):
    """fails without the feature: the entry point, the spec kind, and the size of the accumulators as the library reports it"""
    assert hasattr(emu_lib.dll, "fdtd_add_lattice_dft_monitor") and "fdtd_add_lattice_dft_monitor" in L.SYMBOLS
    spec_d, spec_h = ctx["dd"].spec, ctx["dh"].spec
    assert [m.kind for m in spec_d.monitors] == ["dft_lattice"] * N_SURF and [m.kind for m in spec_h.monitors] == ["dft"] * N_SURF
    assert [m.name for m in spec_d.monitors] == [m.name for m in spec_h.monitors]
    for a, b in zip(spec_d.monitors, spec_h.monitors):      # the same padded box, steps and phase tables
        assert (a.comps, a.lo, a.hi) == (b.comps, b.lo, b.hi) and np.array_equal(a.steps, b.steps) and a.stride == b.stride
        assert np.array_equal(a.phase_e, b.phase_e) and np.array_equal(a.phase_h, b.phase_h) and len(a.freqs) == 3
    with HipEngine(spec_d, lib=emu_lib, axis_shift=0) as ed, HipEngine(spec_h, lib=emu_lib, axis_shift=0) as eh:
        for plan in ctx["dd"].plans:
            n = plan.monitor.name
            nodes = sum(int(np.prod([len(p) for p in pts])) for pts in plan.lattices)
            d, host = ed.monitor_bytes(n, detail=True), eh.monitor_bytes(n, detail=True)
            assert d["series"] == 3 * 4 * nodes * 8 == case.lattice_bytes(ctx["dd"], n) and d["records"] == 0, (n, d)
            cells = sum(int(np.prod(m.shape)) for m in spec_h.monitors if m.name.split("::")[0] == n)
            assert host["records"] == 3 * 4 * cells * 8 and host["series"] == 0, (n, host)
            print(f"[projection_dft] {n}: accumulators {d['series']} B on the device path, {host['records']} B on the host path")
            # the tables: four taps (index + weight) per lattice node, axis and component, and the two phase tables per surface
            mons = [m for m in spec_d.monitors if m.name.split("::")[0] == n]
            assert d["tables"] == sum(32 * len(t[a][0]) for m in mons for t in m.taps for a in range(3)) + sum(2 * 8 * len(m.steps) * 3 for m in mons), (n, d)
            assert d["total"] == d["series"] + d["tables"], (n, d)


def test_the_case_holds_every_kind_of_tap_table(ctx):
    from tidy3d_amd.data import colocation_taps, lattice_taps
    mons = {m.name: m for m in ctx["dd"].spec.monitors}
    plans = {p.monitor.name: p for p in ctx["dd"].plans}
    # all three orientations; on the surfaces normal to x a component keeps one node along x
    assert [mons[f"box::{s}"].targets[0].index(1) for s in ("x-", "x+", "y-", "y+", "z-", "z+")] == [0, 0, 1, 1, 2, 2]
    assert mons["med::plane"].targets[0][0] == 1 and mons["med::plane"].targets[0][1] > 1
    for m in mons.values():
        fp = [f for p in plans.values() for f in p.fields if f.spec_name == m.name][0]
        pts = plans[m.name.split("::")[0]].lattices[list(plans[m.name.split("::")[0]].fields).index(fp)]
        ext = tuple(m.hi[a] - m.lo[a] for a in range(3))
        for ic, f in enumerate(fp.fields):
            again, colo = lattice_taps(ctx["dd"].spec, fp, f, ext, pts), colocation_taps(ctx["dd"].spec, fp, f, ext)
            for a in range(3):
                j, w = m.taps[ic][a]
                assert j.dtype == np.int32 and w.dtype == np.float64 and j.shape == w.shape == (len(pts[a]), 4), (m.name, f, a)
                assert np.array_equal(j, again[a][0]) and np.array_equal(w, again[a][1])
                assert j.min() >= 0 and j.max() < ext[a] and (w >= 0).all() and (w.sum(axis=1) <= 1 + 1e-12).all(), (m.name, f, a)
                # the slots: node j tap 0, node j tap 1, node j + 1 tap 0, node j + 1 tap 1 — every pair is a row of the colocation table
                rows = {tuple(r) for r in colo[a][0].tolist()}
                assert all(tuple(r[:2]) in rows and tuple(r[2:]) in rows for r in j.tolist()), (m.name, f, a)
        # the normal axis: one node, its two colocation taps, two slots of weight 0
        n_ax = m.targets[0].index(1)
        assert all(t[n_ax][1].shape == (1, 4) and not t[n_ax][1][0, 2:].any() for t in m.taps), m.name
    # ksp: the lattice is clipped to the domain; its box goes around the whole periodic z axis and the closing samples wrap
    sim = ctx["dd"].sim
    px, _, pz = plans["ksp"].lattices[0]
    assert px[0] == sim.center[0] - 0.5 * sim.size[0] and px[-1] == sim.center[0] + 0.5 * sim.size[0]
    assert mons["ksp::plane"].lo[2] == 0 and mons["ksp::plane"].hi[2] == 32
    jz = mons["ksp::plane"].taps[0][2][0]
    assert any(r[0] == 31 and r[1] == 0 for r in jz[:, :2].tolist() + jz[:, 2:].tolist())
    # med: a lattice finer than the grid — several lattice points between the same two nodes (repeated rows of indices)
    jy = mons["med::plane"].taps[0][1][0]
    assert len(jy) > mons["med::plane"].hi[1] - mons["med::plane"].lo[1] and len(np.unique(jy, axis=0)) < len(jy)
    # top: the box reaches the PEC wall; Ex (on the grid lines along y) takes its upper sample on the wall: weight 0, index in the box
    top = mons["top::plane"]
    assert top.hi[1] == 36 and top.comps[0] == 0
    jy, wy = top.taps[0][1]
    assert wy[0, 1] == 0 and 0 < wy[0, 0] < 1 and jy[0, 1] == top.hi[1] - top.lo[1] - 1
    # the graded axis: the weights along y differ from node to node
    assert len(np.unique(np.round(mons["box::z-"].taps[0][1][1][:, 0], 9))) > 3


def test_device_values_match_the_host_path(ctx):
    a, b = case.lattice_values(ctx["dd"], ctx["raw_a"]), case.lattice_values(ctx["dh"], ctx["raw_b"])
    assert len(b) == 4 * N_SURF and all(np.abs(v).max() > 0 for v in b.values())
    worst, at = case.worst_host_ratio(a, b, case.box_scales(ctx["dh"], ctx["raw_b"]))
    print(f"[projection_dft] device against host path: worst |dA - dB| / A = {worst / case.EPS32:.3f} x 2^-24 at {at} (bar {case.HOST_BAR / case.EPS32:g} x 2^-24)")
    assert worst <= case.HOST_BAR, (worst / case.EPS32, at)


def test_device_values_match_the_oracle(ctx):
    from oracle.fdtd_numpy import OracleFdtd
    ref = case.lattice_values(ctx["dh"], OracleFdtd(ctx["dh"].spec).run(), dtype=np.complex128)
    host, at_h = case.worst_oracle_ratio(case.lattice_values(ctx["dh"], ctx["raw_b"]), ref)
    print(f"[projection_dft] host path against the fp64 oracle: worst |dB - oracle| / field scale = {host:.3e} at {at_h} (bar {case.ORACLE_BAR:.0e})")
    assert host <= case.ORACLE_BAR, (host, at_h)
    worst, at = case.worst_oracle_ratio(case.lattice_values(ctx["dd"], ctx["raw_a"]), ref)
    print(f"[projection_dft] device against the fp64 oracle: worst |dA - oracle| / field scale = {worst:.3e} at {at} (bar {case.ORACLE_BAR:.0e})")
    assert worst <= case.ORACLE_BAR, (worst, at)


def end_result(lib, tmp_path):
    """web.run on both paths: the six spherical components, the containers, the log and the .hdf5 files"""
    from tidy3d_amd import hdf5io, web
    out = {}
    for dev in (True, False):
        path = str(tmp_path / f"proj_{int(dev)}.hdf5")
        out[dev] = (web.run(case.simulation(), n_steps=case.N_STEPS, lib=lib, verbose=False, projection_device=dev, return_tidy3d=False, path=path), path)
    (sa, pa), (sb, pb) = out[True], out[False]
    assert "Projection monitor accumulated on its lattice on the device: box, cart, ksp, med, top." in sa.log and "on its lattice" not in sb.log
    worst, at = case.worst_end_ratio(sa, sb)
    print(f"[projection_dft] web.run, projected fields, device against host path: worst |dA - dB| / largest component = {worst / case.EPS32:.3f} x 2^-24 "
          f"at {at} (bar {case.END_BAR / case.EPS32:g} x 2^-24)")
    assert worst <= case.END_BAR, (worst / case.EPS32, at)
    # the files: the same groups, shapes, dtypes, coordinates and model; only the projected values (and the log's timings) differ
    ta, tb = hdf5io.read_tree(pa), hdf5io.read_tree(pb)
    assert list(ta) == list(tb)
    for k in ta:
        if k == "/JSON_STRING":
            ja, jb = json.loads(ta[k]), json.loads(tb[k])
            ja.pop("log"), jb.pop("log")
            assert ja == jb
        else:
            xa, xb = np.asarray(ta[k]), np.asarray(tb[k])
            assert xa.dtype == xb.dtype and xa.shape == xb.shape, k
            if not k.endswith("__xarray_dataarray_variable__"):
                assert np.array_equal(xa, xb), k
    back = web.load(pa)
    assert all(np.array_equal(np.asarray(getattr(back[n], c).values), np.asarray(getattr(sa[n], c).values), equal_nan=True) for n in case.NAMES for c in case.SPHERICAL)


def test_end_result_and_files(emu_lib, tmp_path):
    end_result(emu_lib, tmp_path)


def test_values_are_bit_identical_across_schedules(ctx, emu_lib):
    two_pass, st = case.run_engine(ctx["dd"].spec, emu_lib, variant=L.VARIANT_ZMARCH)
    assert int(st.fused2_pairs) == 0
    case.same_bits(two_pass, ctx["raw_a"])
    pairs, st = case.run_engine(ctx["dd"].spec, emu_lib, twostep=case.TWOSTEP_WORD)
    print(f"[projection_dft] forced step pairs: fused2_pairs={int(st.fused2_pairs)} off_reason={int(st.fused2_off_reason)}")
    assert int(st.fused2_pairs) > 0
    case.same_bits(pairs, ctx["raw_a"])


@pytest.mark.parametrize("shift", [1, 2])
def test_renamed_axes(ctx, emu_lib, shift):
    """the engine's cyclic axis renaming: taps and node counts renamed with the axes (the lane axis with them), the result un-renamed,
    the passes in the user's order (FDTD_OPT_AXIS_SHIFT) — the bits of the plain layout"""
    raw, _ = case.run_engine(ctx["dd"].spec, emu_lib, axis_shift=shift)
    assert all(np.ndim(v) == 2 for v in raw.values())
    case.same_bits(raw, ctx["raw_a"])


def test_late_monitor_reset_and_reads_in_mid_run(ctx, emu_lib):
    """Lattice DFT monitors added to a live handle after 20 steps accumulate from then on: the bits of a fresh handle whose monitors'
    `steps` (and phase tables) start at step 20.  A read in mid-run does not disturb later records; fdtd_reset and a rerun reproduce
    everything (the late monitors then record from step 0)."""
    spec = ctx["dd"].spec
    names = [m.name for m in spec.monitors]
    late = [m for m in spec.monitors if m.name in ("box::x+", "med::plane", "ksp::plane")]
    late_names = [m.name for m in late]
    tails = []
    for m in late:
        k = int(np.searchsorted(m.steps, 20))
        assert 0 < k < len(m.steps)
        tails.append(dataclasses.replace(m, steps=m.steps[k:], phase_e=m.phase_e[k:], phase_h=m.phase_h[k:]))
    fresh, _ = case.run_engine(dataclasses.replace(spec, monitors=tails), emu_lib)
    with HipEngine(dataclasses.replace(spec, monitors=[m for m in spec.monitors if m not in late]), lib=emu_lib, axis_shift=0,
                   variant=L.VARIANT_FUSED) as e:
        e.set_option(L.OPT_TWOSTEP, 0)
        e.run(20)
        e.add_monitors(late)
        e.run(11)
        mid = e.results()                  # step 31
        assert all(mid[n].any() for n in names) and not np.array_equal(mid["box::z-"], ctx["raw_a"]["box::z-"])
        e.run(case.N_STEPS - 31)
        got = e.results()
        case.same_bits({n: got[n] for n in late_names}, fresh)
        assert not np.array_equal(got["med::plane"], ctx["raw_a"]["med::plane"])
        case.same_bits({n: got[n] for n in names if n not in late_names}, {n: ctx["raw_a"][n] for n in names if n not in late_names})
        e.reset()
        e.run()
        case.same_bits(e.results(), ctx["raw_a"])


def nan_under_zero_weight(spec, lib):
    """A slot of weight 0 is not read.  Ex of `top` alone, recorded at step 0 (E^0 is what set_field wrote) with phase 1, with every
    zero-weight slot along y and z pointed at row 0 / plane 0 of the box — which no slot of non-zero weight reads — and that row and
    plane of the field set to NaN.  Four slots per axis: the wall's slot along y, the two unused slots of the normal axis, and along
    z the slots of lattice points that coincide with a node."""
    top = [m for m in spec.monitors if m.name == "top::plane"][0]
    ix, (iy, wy), (iz, wz) = top.taps[0]
    assert top.comps[0] == 0 and (wy == 0).sum() >= 3 and not (iy[wy != 0] == 0).any()
    keep_z = wz.copy()
    keep_z[iz == 0] = 0.0                   # (plane 0 of the box is given up: the slots that read it get weight 0 too)
    assert (keep_z != 0).any(axis=1).all()
    one = np.ones((1, 3), dtype=np.complex128)
    zeroed = lambda j, w: np.where(w == 0, 0, j).astype(np.int32)          # noqa: E731
    m = dataclasses.replace(top, comps=(0,), taps=((ix, (zeroed(iy, wy), wy), (zeroed(iz, keep_z), keep_z)),), steps=np.asarray([0], dtype=np.int64),
                            phase_e=one, phase_h=one)
    nx, ny, nz = spec.shape
    field = np.random.default_rng(5).standard_normal((nz, ny, nx)).astype(np.float32)
    field[:, top.lo[1], :] = np.nan
    field[top.lo[2], :, :] = np.nan
    with HipEngine(dataclasses.replace(spec, monitors=[m], sources=[], decay_every=0), lib=lib, axis_shift=0) as e:
        e.set_field(0, field)
        e.run(1)
        got = e.results()["top::plane"].reshape((3,) + m.targets[0][::-1])
    want = np.nan_to_num(field[top.lo[2]:top.hi[2], top.lo[1]:top.hi[1], top.lo[0]:top.hi[0]].astype(np.float64))
    scale = np.abs(want).max()
    for axis, (j, w) in ((2, ix), (1, (iy, wy)), (0, (iz, keep_z))):
        shp = [1, 1, 1]
        shp[axis] = -1
        want = sum(np.take(want, np.clip(j[:, t], 0, want.shape[axis] - 1), axis=axis) * w[:, t].reshape(shp) for t in range(4))
    assert np.isfinite(got).all() and not got.imag.any() and np.abs(want).max() > 0
    assert np.abs(got.real - want[None]).max() <= case.HOST_BAR * scale


def test_a_nan_under_a_zero_weight_stays_out(ctx, emu_lib):
    nan_under_zero_weight(ctx["dd"].spec, emu_lib)


def test_another_medium_is_refused_not_resampled(ctx):
    """device-path data re-projected in a medium whose lattice differs from the recorded one: a DataError that says so; the recorded
    medium itself, given explicitly, is accepted"""
    from tidy3d_amd import projection
    from tidy3d_amd.data import source_spectrum_fn
    dd = ctx["dd"]
    plan = [p for p in dd.plans if p.monitor.name == "top"][0]
    norm = source_spectrum_fn(dd, dd.sim.normalize_index)
    th, ph = np.asarray([0.8]), np.asarray([1.2])
    with pytest.raises(DataError, match="another lattice.*not re-sampled"):
        projection._far_fields(dd, plan, ctx["raw_a"], norm, th, ph, medium=td.Medium(permittivity=4.0))
    same = projection._far_fields(dd, plan, ctx["raw_a"], norm, th, ph, medium=dd.sim.medium)
    assert np.array_equal(same[0], projection._far_fields(dd, plan, ctx["raw_a"], norm, th, ph)[0])
    # the host path re-samples as it always did
    ph_plan = [p for p in ctx["dh"].plans if p.monitor.name == "top"][0]
    assert np.isfinite(projection._far_fields(ctx["dh"], ph_plan, ctx["raw_b"], norm, th, ph, medium=td.Medium(permittivity=4.0))[0]).all()


def test_default_keeps_the_case_on_the_host(monkeypatch):
    """None: on the device only where the whole-box accumulators of all the monitor's surfaces would exceed FLUX_TIME_HOST_BYTES AND
    the lattice holds fewer nodes than the boxes"""
    sim = case.simulation()
    today = discretize(sim, n_steps=case.N_STEPS, projection_device=False).spec.monitors
    auto = discretize(sim, n_steps=case.N_STEPS).spec.monitors
    assert [m.kind for m in auto] == ["dft"] * N_SURF
    for a, b in zip(auto, today):
        assert (a.name, a.comps, a.lo, a.hi) == (b.name, b.comps, b.lo, b.hi) and np.array_equal(a.steps, b.steps) and a.taps is None
        assert np.array_equal(a.phase_e, b.phase_e) and np.array_equal(a.phase_h, b.phase_h)
    assert [m.kind for m in D.plan_monitors(sim, discretize(sim, n_steps=8).spec, discretize(sim, n_steps=8).tmesh, 5)[1]] == ["dft"] * N_SURF
    monkeypatch.setattr(D, "FLUX_TIME_HOST_BYTES", 1 << 10)
    moved = {m.name: m.kind for m in discretize(sim, n_steps=case.N_STEPS).spec.monitors}
    assert set(moved.values()) == {"dft_lattice"}, moved
    # a lattice that holds MORE nodes than the box (a projection medium of index 10) stays on the host path whatever the threshold
    med = [m for m in sim.monitors if m.name == "med"][0]
    fine = dataclasses.replace(sim, monitors=[dataclasses.replace(med, medium=td.Medium(permittivity=100.0))])
    assert [m.kind for m in discretize(fine, n_steps=8).spec.monitors] == ["dft"]
    assert [m.kind for m in discretize(fine, n_steps=8, projection_device=True).spec.monitors] == ["dft_lattice"]
    from tidy3d_amd import dist
    assert [m.kind for m in dist.slab_discretization(sim, case.N_STEPS).spec.monitors] == ["dft"] * N_SURF
    # only projection monitors move: flux, mode and diffraction monitors keep kind "dft" whatever is asked
    flux = dataclasses.replace(sim, monitors=[td.FluxMonitor(center=(0.18, -0.02, 0.03), size=(0, 0.2, 0.31), name="fx", freqs=case.FREQS)])
    assert [m.kind for m in discretize(flux, n_steps=8, projection_device=True).spec.monitors] == ["dft"]
    per = td.BoundarySpec(x=td.Boundary.periodic(), y=td.Boundary.pml(num_layers=4), z=td.Boundary.periodic())
    diff = dataclasses.replace(sim, boundary_spec=per, monitors=[td.DiffractionMonitor(center=(0, 0.3, 0), size=(td.inf, 0, td.inf), name="d", freqs=case.FREQS)])
    assert [m.kind for m in discretize(diff, n_steps=8, projection_device=True).spec.monitors] == ["dft"]


def test_refusals(emu_lib):
    from tidy3d_amd import web
    sim = case.simulation()
    with pytest.raises(Tidy3dNotImplementedError, match="projection_device=True.*symmetry"):
        discretize(dataclasses.replace(sim, symmetry=(0, 0, 1)), n_steps=8, projection_device=True)
    bloch = td.BoundarySpec(x=td.Boundary.pml(num_layers=4), y=td.Boundary(minus=td.PMCBoundary(), plus=td.PECBoundary()), z=td.Boundary.bloch(0.3))
    with pytest.raises(Tidy3dNotImplementedError, match="projection_device=True.*Bloch"):
        discretize(dataclasses.replace(sim, boundary_spec=bloch), n_steps=8, projection_device=True)
    assert all(m.kind == "dft" for m in discretize(dataclasses.replace(sim, boundary_spec=bloch), n_steps=8).spec.monitors)
    assert all(m.kind == "dft" for m in discretize(dataclasses.replace(sim, symmetry=(0, 0, 1)), n_steps=8).spec.monitors)
    with pytest.raises(Tidy3dNotImplementedError, match="projection_device=True.*more than one GPU"):
        web.run(sim, n_steps=8, lib=emu_lib, verbose=False, projection_device=True, devices=[0, 1])
    spec = discretize(sim, n_steps=8, projection_device=True).spec
    with pytest.raises(SolverLibraryError, match="z-slab"):
        HipEngine(spec, lib=emu_lib, force_comm=True)
    i32 = lambda *v: np.asarray(v, dtype=np.int32)              # noqa: E731
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)             # noqa: E731
    comps, lo, hi, steps = i32(1, 5), i32(2, 2, 2), i32(5, 6, 6), np.asarray([1, 2], dtype=np.int64)
    nt = i32(2, 3, 1, 2, 3, 1)
    idx = np.zeros(2 * 4 * (2 + 3 + 1), dtype=np.int32)
    w = np.tile(np.asarray([0.5, 0.0, 0.5, 0.0], dtype=np.float32), 2 * (2 + 3 + 1))
    ph = np.ones((2, 3, 2), dtype=np.float32)                   # [n_rec][nf] complex64
    add = lambda e, ix, ww, n_taps=4: e.lib.dll.fdtd_add_lattice_dft_monitor(e.handle, 2, p(comps), p(lo), p(hi), 2, p(steps), p(nt), n_taps, p(ix), p(ww), 3, p(ph), p(ph))   # noqa: E731
    # the library itself refuses a z-slab handle, by message, before anything is launched
    with HipEngine(dataclasses.replace(spec, monitors=[]), lib=emu_lib, force_comm=True) as e:
        assert add(e, idx, w) < 0
        assert "fdtd_add_lattice_dft_monitor" in e.lib.error(e.handle) and "z-slab" in e.lib.error(e.handle)
    with HipEngine(dataclasses.replace(spec, monitors=[]), lib=emu_lib, axis_shift=0) as e:
        # the generic entry point refuses the kind and names the right one
        assert e.lib.dll.fdtd_add_monitor(e.handle, L.MON_DFT_LATTICE, 2, p(comps), p(lo), p(hi), 2, p(steps), 3, p(ph), p(ph)) < 0
        assert "fdtd_add_lattice_dft_monitor" in e.lib.error(e.handle)
        # any other number of taps per node
        for n_taps in (2, 3, 8):
            assert add(e, idx, w, n_taps) < 0 and "n_taps must be 4" in e.lib.error(e.handle), n_taps
        # a slot outside the box: index 3 along x of a box of 3 cells (second component), a negative index, a NaN weight
        for at, bad_i, bad_w in ((24, 3, 1.0), (0, -1, 1.0), (10, 0, np.nan)):
            ix, ww = idx.copy(), w.copy()
            ix[at], ww[at] = bad_i, bad_w
            assert add(e, ix, ww) < 0 and "outside the box" in e.lib.error(e.handle), (at, e.lib.error(e.handle))
        # ... but not under a zero weight; and the tables as they are are accepted
        ix = idx.copy()
        ix[25] = 99
        assert add(e, ix, w) == 0 and add(e, idx, w) == 1
        buf = (ctypes.c_int64 * 4)()
        assert e.lib.dll.fdtd_get_monitor_bytes(e.handle, 1, buf) == 0 and buf[1] == 0 and buf[2] == 8 * 3 * 2 * 6
