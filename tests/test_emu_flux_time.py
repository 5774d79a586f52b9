"""FluxTimeMonitor surfaces reduced on the device (MonitorSpec kind "flux_time", csrc/fdtd_flux_time.hpp), on the CPU emulator:
against the host path of the same engine and against the fp64 oracle, bit for bit across schedules, staging rings, fdtd_reset,
monitors added to a live handle and get_field / set_field in mid-run; bounded device memory; the choice between the two paths and
its refusals.  The case and the bars: tests/flux_time_case.py.

Measured (printed by the tests; the emulator and the MI355X give the same figures): worst |device - host| / A_scale = 1.32 x 2^-24
(bar 32 x 2^-24), worst |device - oracle| / A_scale = 2.2e-7 (bar 4e-5)."""
import ctypes
import dataclasses

import numpy as np
import pytest

import tidy3d_amd.schema as td
from tidy3d_amd import discretize as D
from tidy3d_amd import lib as L
from tidy3d_amd.discretize import discretize
from tidy3d_amd.engine import HipEngine
from tidy3d_amd.exceptions import SolverLibraryError, Tidy3dNotImplementedError

import flux_time_case as case


@pytest.fixture(scope="module")
def ctx(emu_lib):
    """the two discretizations, run A (device path, fused single steps) and run B (host path), computed once"""
    dd, dh = case.discs()
    assert [m.kind for m in dd.spec.monitors] == ["flux_time"] * 10 and [m.kind for m in dh.spec.monitors] == ["time"] * 10
    raw_a, _ = case.run_engine(dd.spec, emu_lib)
    raw_b, _ = case.run_engine(dh.spec, emu_lib)
    return dict(dd=dd, dh=dh, raw_a=raw_a, raw_b=raw_b, scale=case.scales(dh, raw_b))


def test_device_series_match_the_host_path(ctx):
    a, b = case.series(ctx["dd"], ctx["raw_a"]), case.series(ctx["dh"], ctx["raw_b"])
    for n in case.NAMES:
        assert a[n].dtype == np.float32 and a[n].shape == b[n].shape and np.abs(b[n]).max() > 0, n
    assert (len(a["px"]), len(a["py"]), len(a["pz"]), len(a["box"]), len(a["win"])) == (57, 19, 19, 19, 23)
    worst, at = case.worst_ratio(a, b, ctx["scale"])
    print(f"[flux_time] device against host path: worst |dA - dB| / A_scale = {worst / case.EPS32:.3f} x 2^-24 at '{at}' (bar 32 x 2^-24)")
    assert worst <= case.HOST_BAR, (worst / case.EPS32, at)


def test_device_series_match_the_oracle(ctx):
    from oracle.fdtd_numpy import OracleFdtd
    ref = case.series(ctx["dh"], OracleFdtd(ctx["dh"].spec).run())
    worst, at = case.worst_ratio(case.series(ctx["dd"], ctx["raw_a"]), ref, ctx["scale"])
    print(f"[flux_time] device against the fp64 oracle: worst |dA - oracle| / A_scale = {worst:.3e} at '{at}' (bar {case.ORACLE_BAR:.0e})")
    assert worst <= case.ORACLE_BAR, (worst, at)


def test_series_are_bit_identical_across_schedules(ctx, emu_lib):
    two_pass, st = case.run_engine(ctx["dd"].spec, emu_lib, variant=L.VARIANT_ZMARCH)
    assert int(st.fused2_pairs) == 0
    case.same_bits(two_pass, ctx["raw_a"])
    pairs, st = case.run_engine(ctx["dd"].spec, emu_lib, twostep=case.TWOSTEP_WORD)
    print(f"[flux_time] forced step pairs: fused2_pairs={int(st.fused2_pairs)} shell_pairs={int(st.shell_pairs)} shell2_pairs={int(st.shell2_pairs)} "
          f"off_reason={int(st.fused2_off_reason)}")
    assert int(st.fused2_pairs) > 0
    case.same_bits(pairs, ctx["raw_a"])


@pytest.mark.parametrize("records", [2, 5])
def test_staging_ring_wraps(ctx, emu_lib, records):
    """rings of exactly 2 and 5 records under 57, 19 and 23 records, single steps and step pairs: the bits of the unbounded ring"""
    spec = case.with_budget(ctx["dd"].spec, records)
    with HipEngine(spec, lib=emu_lib, axis_shift=0, variant=L.VARIANT_FUSED) as e:
        e.set_option(L.OPT_TWOSTEP, 0)
        e.run()
        for n in case.NAMES:
            d = e.monitor_bytes(n, detail=True)
            assert d["records"] == sum(records * 16 * int(np.prod(m.shape)) for m in spec.monitors if m.name.split("::")[0] == n), (n, d)
        case.same_bits(e.results(), ctx["raw_a"])
    got, st = case.run_engine(spec, emu_lib, twostep=case.TWOSTEP_WORD)
    assert int(st.fused2_pairs) > 0
    case.same_bits(got, ctx["raw_a"])


def test_reset_late_monitor_and_field_access(ctx, emu_lib):
    """Flux-time monitors added to a live handle after 20 steps: `win`, whose first record is step 20, gives its whole series; `px`,
    which records from step 3 on, SKIPS the steps already done (fdtd_add_flux_time_monitor: their entries stay zero) and gives the
    tail of the series of a monitor present from the start.  After fdtd_reset both record everything."""
    spec = case.with_budget(ctx["dd"].spec, 5)
    late = [m for m in spec.monitors if m.name.split("::")[0] in ("win", "px")]
    with HipEngine(dataclasses.replace(spec, monitors=[m for m in spec.monitors if m not in late]), lib=emu_lib, axis_shift=0,
                   variant=L.VARIANT_FUSED) as e:
        e.set_option(L.OPT_TWOSTEP, 0)
        e.run(20)
        e.add_monitors(late)
        for c in range(6):                 # all six fields read and written back in mid-run
            e.set_field(c, e.get_field(c))
        e.run(case.N_STEPS - 20)
        got = e.results()
        px = [m for m in late if m.name.startswith("px")][0]
        done = int(np.searchsorted(px.steps, 20))
        assert 0 < done < len(px.steps) and not got[px.name][:done].any()
        full = dict(got)
        full[px.name] = np.concatenate([ctx["raw_a"][px.name][:done], got[px.name][done:]])
        case.same_bits(full, ctx["raw_a"])
        e.reset()
        e.run()
        case.same_bits(e.results(), ctx["raw_a"])


@pytest.mark.parametrize("shift", [1, 2])
def test_renamed_axes(ctx, emu_lib, shift):
    """the engine's cyclic axis renaming (what best_axis_shift chooses on real grids): normal, taps and weights renamed with the axes"""
    raw, _ = case.run_engine(ctx["dd"].spec, emu_lib, axis_shift=shift)
    assert all(np.ndim(v) == 1 for v in raw.values())
    worst, at = case.worst_ratio(case.series(ctx["dd"], raw), case.series(ctx["dh"], ctx["raw_b"]), ctx["scale"])
    print(f"[flux_time] axis shift {shift}: worst |dA - dB| / A_scale = {worst / case.EPS32:.3f} x 2^-24 at '{at}'")
    assert worst <= case.HOST_BAR, (worst / case.EPS32, at)


def test_web_run_forwards_the_choice(ctx, emu_lib):
    from tidy3d_amd import web
    sd = web.run(case.simulation(), n_steps=case.N_STEPS, lib=emu_lib, verbose=False, flux_time_device=True, return_tidy3d=False)
    assert "FluxTimeMonitor reduced on the device: box, px, py, pz, win." in sd.log
    got = {n: np.asarray(sd[n].flux.values) for n in case.NAMES}
    worst, at = case.worst_ratio(got, case.series(ctx["dh"], ctx["raw_b"]), ctx["scale"])
    assert worst <= case.HOST_BAR, (worst / case.EPS32, at)
    host = web.run(case.simulation(), n_steps=case.N_STEPS, lib=emu_lib, verbose=False, return_tidy3d=False)
    assert "reduced on the device" not in host.log
    with pytest.raises(Tidy3dNotImplementedError, match="more than one GPU"):
        web.run(case.simulation(), n_steps=8, lib=emu_lib, verbose=False, flux_time_device=True, devices=[0, 1])


def test_z_slab_runs_keep_the_host_path(monkeypatch, emu_lib):
    """the distributed entry point never chooses the device reduction, however large the records"""
    from tidy3d_amd import dist
    monkeypatch.setattr(D, "FLUX_TIME_HOST_BYTES", 1 << 10)
    sim = case.simulation()
    assert all(m.kind == "flux_time" for m in discretize(sim, n_steps=case.N_STEPS).spec.monitors)
    spec = dist.slab_discretization(sim, case.N_STEPS).spec
    assert [m.kind for m in spec.monitors] == ["time"] * 10
    with HipEngine(spec, lib=emu_lib, force_comm=True) as e:
        assert len(e.mon_ids) == 10


def test_device_memory_is_bounded(ctx, emu_lib):
    spec_d, spec_h = ctx["dd"].spec, ctx["dh"].spec
    with HipEngine(spec_d, lib=emu_lib, axis_shift=0) as ed, HipEngine(spec_h, lib=emu_lib, axis_shift=0) as eh:
        for n in case.NAMES:
            surf = [m for m in spec_d.monitors if m.name.split("::")[0] == n]
            d, host = ed.monitor_bytes(n, detail=True), eh.monitor_bytes(n)
            n_rec = len(surf[0].steps)
            cells = [int(np.prod(m.shape)) for m in surf]
            # the staging ring (here every record fits the default budget: n_rec records) plus n_rec floats per surface ...
            assert d["records"] == sum(n_rec * 16 * c for c in cells) and d["series"] == 4 * n_rec * len(surf), (n, d)
            # ... and the tables: per axis two taps (index + weight) per component and node, one weight per node, one partial per ring slot and tile
            tables = 0
            for m in surf:
                nodes = [len(w) for w in m.weights]
                tables += sum(4 * (2 * 8 * k + k) for k in nodes) + 4 * n_rec * (-(-int(np.prod(nodes)) // 1024))
            assert d["tables"] == tables and d["total"] == d["records"] + d["series"] + d["tables"], (n, d, tables)
            assert host == sum(n_rec * 16 * c for c in cells)
    # a budget of two records: the ring, not the number of records, bounds the allocation
    with HipEngine(case.with_budget(spec_d, 2), lib=emu_lib, axis_shift=0) as e:
        for n in case.NAMES:
            surf = [m for m in spec_d.monitors if m.name.split("::")[0] == n]
            d = e.monitor_bytes(n, detail=True)
            assert d["records"] == sum(2 * 16 * int(np.prod(m.shape)) for m in surf) and d["series"] == 4 * len(surf[0].steps) * len(surf), (n, d)


def test_default_keeps_small_monitors_on_the_host(monkeypatch):
    sim = case.simulation()
    today = discretize(sim, n_steps=case.N_STEPS, flux_time_device=False).spec.monitors
    auto = discretize(sim, n_steps=case.N_STEPS).spec.monitors
    assert [m.kind for m in auto] == ["time"] * len(today)
    for a, b in zip(auto, today):
        assert (a.name, a.comps, a.lo, a.hi) == (b.name, b.comps, b.lo, b.hi) and np.array_equal(a.steps, b.steps) and a.taps is None
    monkeypatch.setattr(D, "FLUX_TIME_HOST_BYTES", 1 << 10)
    moved = discretize(sim, n_steps=case.N_STEPS).spec.monitors
    assert [m.kind for m in moved] == ["flux_time"] * len(today) and [m.name for m in moved] == [m.name for m in today]


def test_refusals(emu_lib):
    sim = case.simulation()
    with pytest.raises(Tidy3dNotImplementedError, match="symmetry"):
        discretize(dataclasses.replace(sim, symmetry=(0, 0, 1)), n_steps=8, flux_time_device=True)
    bloch = td.BoundarySpec(x=td.Boundary.pml(num_layers=4), y=td.Boundary(minus=td.PMCBoundary(), plus=td.PECBoundary()), z=td.Boundary.bloch(0.3))
    with pytest.raises(Tidy3dNotImplementedError, match="Bloch"):
        discretize(dataclasses.replace(sim, boundary_spec=bloch), n_steps=8, flux_time_device=True)
    assert all(m.kind == "time" for m in discretize(dataclasses.replace(sim, boundary_spec=bloch), n_steps=8).spec.monitors)
    assert all(m.kind == "time" for m in discretize(dataclasses.replace(sim, symmetry=(0, 0, 1)), n_steps=8).spec.monitors)
    spec = discretize(sim, n_steps=8, flux_time_device=True).spec
    with pytest.raises(SolverLibraryError, match="z-slab"):
        HipEngine(spec, lib=emu_lib, force_comm=True)
    # the library itself refuses a z-slab handle, by message, before anything is launched
    with HipEngine(dataclasses.replace(spec, monitors=[]), lib=emu_lib, force_comm=True) as e:
        i32, f32 = (lambda *v: np.asarray(v, dtype=np.int32)), (lambda *v: np.asarray(v, dtype=np.float32))
        lo, hi, nn, steps = i32(2, 2, 2), i32(3, 6, 6), i32(1, 4, 4), np.asarray([1, 2], dtype=np.int64)
        idx, w, wu = np.zeros(8 * 9, dtype=np.int32), np.zeros(8 * 9, dtype=np.float32), f32(1, 1, 1, 1)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)         # noqa: E731
        assert e.lib.dll.fdtd_add_flux_time_monitor(e.handle, 0, 1.0, p(lo), p(hi), 2, p(steps), p(nn), p(idx), p(w), p(wu), p(wu), 0) < 0
        assert "fdtd_add_flux_time_monitor" in e.lib.error(e.handle) and "z-slab" in e.lib.error(e.handle)
        comps = i32(1, 2, 4, 5)
        assert e.lib.dll.fdtd_add_monitor(e.handle, L.MON_FLUX_TIME, 4, p(comps), p(lo), p(hi), 2, p(steps), 0, None, None) < 0
        assert "fdtd_add_flux_time_monitor" in e.lib.error(e.handle)
