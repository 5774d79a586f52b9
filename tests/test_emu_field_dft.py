"""FieldMonitor DFTs accumulated on the kept nodes only, on the device (MonitorSpec kind "dft_sparse", csrc/fdtd_field_dft.hpp), on the
CPU emulator: against the host path of the same engine and against the fp64 oracle, bit for bit across schedules, the engine's axis
renaming, fdtd_reset, monitors added to a live handle and reads in mid-run; the device memory the library reports; the choice
between the two paths and its refusals.  The case and the bars: tests/field_dft_case.py.

Measured (printed by the tests; the emulator and the MI355X give the same figures): worst |device - host| / A = 2.435 x 2^-24 at
('win', 'Ey') (bar 16 x 2^-24: the figure times 4, rounded up to a power of two); `yee` and `sml` (colocate=False: weights 1 / 0)
are bit-identical to the host path.  Against the fp64 oracle: host path 1.655e-5, device path 1.655e-5 of the component's
largest value (bar 2e-5)."""
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

import field_dft_case as case


@pytest.fixture(scope="module")
def ctx(emu_lib):
    """the two discretizations, run A (device path, fused single steps) and run B (host path), computed once"""
    dd, dh = case.discs()
    raw_a, _ = case.run_engine(dd.spec, emu_lib)
    raw_b, _ = case.run_engine(dh.spec, emu_lib)
    return dict(dd=dd, dh=dh, raw_a=raw_a, raw_b=raw_b)


def test_the_feature_is_there(ctx, emu_lib):
    """fails without the feature: the spec kind, the entry point, and the size of the accumulators as the library reports it"""
    spec_d, spec_h = ctx["dd"].spec, ctx["dh"].spec
    assert [m.kind for m in spec_d.monitors] == ["dft_sparse"] * 6 and [m.kind for m in spec_h.monitors] == ["dft"] * 6
    assert [m.name for m in spec_d.monitors] == list(case.NAMES)
    assert hasattr(emu_lib.dll, "fdtd_add_field_dft_monitor")
    with HipEngine(spec_d, lib=emu_lib, axis_shift=0) as ed, HipEngine(spec_h, lib=emu_lib, axis_shift=0) as eh:
        for m, mh in zip(spec_d.monitors, spec_h.monitors):
            d, host = ed.monitor_bytes(m.name, detail=True), eh.monitor_bytes(m.name, detail=True)
            want = 8 * len(m.freqs) * sum(int(np.prod([len(t[a][0]) for a in range(3)])) for t in m.taps)
            assert len(m.freqs) == 3 and want == case.accumulator_bytes(m) and d["series"] == want and d["records"] == 0, (m.name, d, want)
            assert host["records"] == 8 * len(mh.freqs) * len(mh.comps) * int(np.prod(mh.shape)) and host["series"] == 0, (m.name, host)
            print(f"[field_dft] {m.name}: accumulators {d['series']} B on the device path, {host['records']} B on the host path")
            if m.name != "sml":            # (a box of a few cells: nothing is asked of it)
                assert d["series"] < host["records"], (m.name, d, host)
            # the tables: two taps (index + weight) per kept node and axis, and the two phase tables
            assert d["tables"] == sum(16 * len(t[a][0]) for t in m.taps for a in range(3)) + 2 * 8 * len(m.steps) * len(m.freqs), (m.name, d)
            assert d["total"] == d["series"] + d["tables"], (m.name, d)


def test_the_case_holds_every_kind_of_tap_table(ctx):
    mons = {m.name: m for m in ctx["dd"].spec.monitors}
    assert ctx["dd"].nyquist_step > 2 and np.array_equal(mons["vol"].steps, np.arange(0, case.N_STEPS, ctx["dd"].nyquist_step))
    assert np.array_equal(mons["win"].steps, np.arange(0, case.N_STEPS, 2)) and mons["win"].stride == 2 and mons["win"].apod is not None
    # the window rides in the phase tables: its ramps are there
    mag = np.abs(mons["win"].phase_e[:, 0])
    assert mag[0] < 0.1 * mag.max() and mag[-1] < 0.5 * mag.max() and np.ptp(np.abs(mons["vol"].phase_e[:, 0])) < 1e-12 * mag.max()
    assert len(mons["vol"].comps) == 6 and any(0 < w < 1 for w in np.asarray(mons["vol"].taps[1][1][1]).ravel())
    # yee, sml: weights 1 / 0 only
    assert all(set(np.unique(t[a][1])) <= {0.0, 1.0} for n in ("yee", "sml") for t in mons[n].taps for a in range(3))
    assert mons["sml"].shape == (6, 6, 6)
    # pln: both taps along the normal carry weight; the last node along the periodic axis takes its second tap from the other end
    ix, wx = mons["pln"].taps[0][0]
    assert ix.shape == (1, 2) and 0 < wx[0, 0] < 1 and 0 < wx[0, 1] < 1
    iz, wz = mons["pln"].taps[0][2]
    assert iz[-1].tolist() == [31, 0] and wz[-1, 1] > 0 and mons["pln"].lo[2] == 0 and mons["pln"].hi[2] == 32
    # top: its last node lies ON the PEC wall (Ex is zero there): the tap on the wall has been clipped into the box and carries weight 0
    iy, wy = mons["top"].taps[0][1]
    assert mons["top"].hi[1] == 36 and iy[-1].tolist() == [mons["top"].shape[1] - 1] * 2 and wy[-1].tolist() == [0.0, 0.0]
    assert (wy[:-1].sum(axis=1) == 1.0).all()


def test_device_values_match_the_host_path(ctx):
    a, b = case.fields(ctx["dd"], ctx["raw_a"]), case.fields(ctx["dh"], ctx["raw_b"])
    assert len(b) == 18 and all(np.abs(v).max() > 0 for v in b.values())
    worst, at, same = case.worst_host_ratio(a, b, case.box_scales(ctx["dh"], ctx["raw_b"]))
    print(f"[field_dft] device against host path: worst |dA - dB| / A = {worst / case.EPS32:.3f} x 2^-24 at {at} (bar {case.HOST_BAR / case.EPS32:g} x 2^-24)")
    print("[field_dft] share of bit-identical values: " + ", ".join(f"{k[0]}.{k[1]} {v:.3f}" for k, v in same.items()))
    # weights 1 / 0: the device accumulates the very samples the host path's accumulators of those nodes take
    assert all(same[k] == 1.0 for k in same if k[0] in ("yee", "sml")), same
    assert worst <= case.HOST_BAR, (worst / case.EPS32, at)
    # the containers themselves: same coordinates, same dtype
    from tidy3d_amd.data import assemble
    sa, sb = assemble(ctx["dd"], ctx["raw_a"]), assemble(ctx["dh"], ctx["raw_b"])
    for n in case.NAMES:
        for f in ("Ex", "Ey", "Ez", "Hx", "Hy", "Hz"):
            xa, xb = getattr(sa[n], f), getattr(sb[n], f)
            assert (xa is None) == (xb is None), (n, f)
            if xa is not None:
                assert xa.values.dtype == xb.values.dtype == np.complex64 and xa.values.shape == xb.values.shape and list(xa.coords) == list(xb.coords), (n, f)
                assert all(np.array_equal(np.asarray(xa.coords[k]), np.asarray(xb.coords[k])) for k in xa.coords), (n, f)


def test_device_values_match_the_oracle(ctx):
    from oracle.fdtd_numpy import OracleFdtd
    ref = case.fields(ctx["dh"], OracleFdtd(ctx["dh"].spec).run(), dtype=np.complex128)
    host, at_h = case.worst_oracle_ratio(case.fields(ctx["dh"], ctx["raw_b"]), ref)
    print(f"[field_dft] host path against the fp64 oracle: worst |dB - oracle| / field scale = {host:.3e} at {at_h} (bar {case.ORACLE_BAR:.0e})")
    assert host <= case.ORACLE_BAR, (host, at_h)
    worst, at = case.worst_oracle_ratio(case.fields(ctx["dd"], ctx["raw_a"]), ref)
    print(f"[field_dft] device against the fp64 oracle: worst |dA - oracle| / field scale = {worst:.3e} at {at} (bar {case.ORACLE_BAR:.0e})")
    assert worst <= case.ORACLE_BAR, (worst, at)


def test_values_are_bit_identical_across_schedules(ctx, emu_lib):
    two_pass, st = case.run_engine(ctx["dd"].spec, emu_lib, variant=L.VARIANT_ZMARCH)
    assert int(st.fused2_pairs) == 0
    case.same_bits(two_pass, ctx["raw_a"])
    pairs, st = case.run_engine(ctx["dd"].spec, emu_lib, twostep=case.TWOSTEP_WORD)
    print(f"[field_dft] forced step pairs: fused2_pairs={int(st.fused2_pairs)} off_reason={int(st.fused2_off_reason)}")
    assert int(st.fused2_pairs) > 0            # (`win` records at every even step: the first step of every pair, so every pair feeds the kernel from the dump)
    case.same_bits(pairs, ctx["raw_a"])


@pytest.mark.parametrize("shift", [1, 2])
def test_renamed_axes(ctx, emu_lib, shift):
    """the engine's cyclic axis renaming: taps and kept-node counts renamed with the axes, the result un-renamed, the passes in the
    user's order (FDTD_OPT_AXIS_SHIFT) — the bits of the plain layout"""
    raw, _ = case.run_engine(ctx["dd"].spec, emu_lib, axis_shift=shift)
    assert all(np.ndim(v) == 2 for v in raw.values())
    case.same_bits(raw, ctx["raw_a"])


def test_late_monitor_reset_and_reads_in_mid_run(ctx, emu_lib):
    """Sparse DFT monitors added to a live handle after 20 steps accumulate from then on: the bits of a fresh handle whose monitors'
    `steps` (and phase tables) start at step 20.  A read in mid-run does not disturb later records; fdtd_reset and a rerun reproduce
    everything (the late monitors then record from step 0)."""
    spec = ctx["dd"].spec
    late = [m for m in spec.monitors if m.name in ("win", "sml")]
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
        assert all(mid[n].any() for n in case.NAMES) and not np.array_equal(mid["vol"], ctx["raw_a"]["vol"])
        e.run(case.N_STEPS - 31)
        got = e.results()
        case.same_bits({n: got[n] for n in ("win", "sml")}, fresh)
        assert not np.array_equal(got["win"], ctx["raw_a"]["win"])
        case.same_bits({n: got[n] for n in case.NAMES if n not in ("win", "sml")}, {n: ctx["raw_a"][n] for n in case.NAMES if n not in ("win", "sml")})
        e.reset()
        e.run()
        case.same_bits(e.results(), ctx["raw_a"])


def test_components_may_keep_different_node_counts(ctx, emu_lib):
    """the layout of the result — the components of a frequency one after the other, each with its own extents — with a hand-made
    spec: `yee` with the last kept x node of Hz and the first kept z node of Ex taken away"""
    yee = [m for m in ctx["dd"].spec.monitors if m.name == "yee"][0]
    (ex_x, ex_y, ex_z), (hz_x, hz_y, hz_z) = yee.taps
    cut = dataclasses.replace(yee, taps=((ex_x, ex_y, (ex_z[0][1:], ex_z[1][1:])), ((hz_x[0][:-1], hz_x[1][:-1]), hz_y, hz_z)))
    (nx, ny, nz), (mx, my, mz) = yee.targets
    assert cut.targets == ((nx, ny, nz - 1), (mx - 1, my, mz)) and nx * ny * (nz - 1) != (mx - 1) * my * mz
    raw, _ = case.run_engine(dataclasses.replace(ctx["dd"].spec, monitors=[cut]), emu_lib)
    full = ctx["raw_a"]["yee"]
    ex, hz = full[:, :nx * ny * nz].reshape(3, nz, ny, nx), full[:, nx * ny * nz:].reshape(3, mz, my, mx)
    want = np.concatenate([ex[:, 1:].reshape(3, -1), hz[..., :-1].reshape(3, -1)], axis=1)
    assert raw["yee"].shape == (3, nx * ny * (nz - 1) + (mx - 1) * my * mz)
    case.same_bits({"yee": raw["yee"]}, {"yee": np.ascontiguousarray(want)})


def nan_under_zero_weight(spec, lib):
    """A tap of weight 0 is not read.  Ex of `top` alone, recorded at step 0 (E^0 is what set_field wrote) with phase 1, with every
    zero-weight tap along y pointed at row 0 of the box — which no tap of non-zero weight reads — and that row of the field set to NaN."""
    top = [m for m in spec.monitors if m.name == "top"][0]
    ix, (iy, wy), iz = top.taps[0]
    assert top.comps[0] == 0 and (wy == 0).any() and not (iy[wy != 0] == 0).any()
    one = np.ones((1, 3), dtype=np.complex128)
    m = dataclasses.replace(top, comps=(0,), taps=((ix, (np.where(wy == 0, 0, iy).astype(np.int32), wy), iz),), steps=np.asarray([0], dtype=np.int64),
                            phase_e=one, phase_h=one)
    nx, ny, nz = spec.shape
    field = np.random.default_rng(5).standard_normal((nz, ny, nx)).astype(np.float32)
    field[:, top.lo[1], :] = np.nan
    with HipEngine(dataclasses.replace(spec, monitors=[m], sources=[], decay_every=0), lib=lib, axis_shift=0) as e:
        e.set_field(0, field)
        e.run(1)
        got = e.results()["top"].reshape((3,) + m.targets[0][::-1])
    box = np.nan_to_num(field[top.lo[2]:top.hi[2], top.lo[1]:top.hi[1], top.lo[0]:top.hi[0]].astype(np.float64))
    want = box
    for axis, (j, w) in ((2, ix), (1, (iy, wy)), (0, iz)):
        shp = [1, 1, 1]
        shp[axis] = -1
        want = np.take(want, j[:, 0], axis=axis) * w[:, 0].reshape(shp) + np.take(want, np.clip(j[:, 1], 0, want.shape[axis] - 1), axis=axis) * w[:, 1].reshape(shp)
    assert np.isfinite(got).all() and not got.imag.any() and np.abs(got.real - want[None]).max() <= case.HOST_BAR * np.abs(box).max()


def test_a_nan_under_a_zero_weight_stays_out(ctx, emu_lib):
    nan_under_zero_weight(ctx["dd"].spec, emu_lib)


def test_web_run_forwards_the_choice(emu_lib):
    from tidy3d_amd import web
    sd = web.run(case.simulation(), n_steps=case.N_STEPS, lib=emu_lib, verbose=False, field_dft_device=True, return_tidy3d=False)
    assert "FieldMonitor accumulated on the device: pln, sml, top, vol, win, yee." in sd.log
    # the engine run of the same discretization (every monitor at the Nyquist step: web.run knows no other), assembled alike
    from tidy3d_amd.data import assemble
    disc = discretize(case.simulation(), n_steps=case.N_STEPS, field_dft_device=True)
    ref = assemble(disc, case.run_engine(disc.spec, emu_lib)[0])
    for plan in disc.plans:
        for f in plan.fields[0].fields:
            got, want = np.asarray(getattr(sd[plan.monitor.name], f).values), np.asarray(getattr(ref[plan.monitor.name], f).values)
            assert got.dtype == np.complex64 and np.array_equal(case.bits(got), case.bits(want)), (plan.monitor.name, f)
    host = web.run(case.simulation(), n_steps=case.N_STEPS, lib=emu_lib, verbose=False, return_tidy3d=False)
    assert "accumulated on the device" not in host.log
    with pytest.raises(Tidy3dNotImplementedError, match="field_dft_device=True.*more than one GPU"):
        web.run(case.simulation(), n_steps=8, lib=emu_lib, verbose=False, field_dft_device=True, devices=[0, 1])


def test_default_keeps_the_case_on_the_host(monkeypatch):
    """None: on the device only where the accumulators of the whole box would exceed FLUX_TIME_HOST_BYTES AND fewer nodes are kept"""
    sim = case.simulation()
    today = discretize(sim, n_steps=case.N_STEPS, field_dft_device=False).spec.monitors
    auto = discretize(sim, n_steps=case.N_STEPS).spec.monitors
    assert [m.kind for m in auto] == ["dft"] * 6
    for a, b in zip(auto, today):
        assert (a.name, a.comps, a.lo, a.hi) == (b.name, b.comps, b.lo, b.hi) and np.array_equal(a.steps, b.steps) and a.taps is None
        assert np.array_equal(a.phase_e, b.phase_e) and np.array_equal(a.phase_h, b.phase_h)
    monkeypatch.setattr(D, "FLUX_TIME_HOST_BYTES", 1 << 10)
    moved = discretize(sim, n_steps=case.N_STEPS).spec.monitors
    assert [m.kind for m in moved] == ["dft_sparse"] * 6
    from tidy3d_amd import dist
    assert [m.kind for m in dist.slab_discretization(sim, case.N_STEPS).spec.monitors] == ["dft"] * 6
    # only FieldMonitors move: a flux monitor's surfaces keep kind "dft" whatever is asked
    flux = dataclasses.replace(sim, monitors=[td.FluxMonitor(center=(0.18, -0.02, 0.03), size=(0, 0.2, 0.31), name="fx", freqs=case.FREQS)])
    assert [m.kind for m in discretize(flux, n_steps=8, field_dft_device=True).spec.monitors] == ["dft"]


def test_refusals(emu_lib):
    sim = case.simulation()
    with pytest.raises(Tidy3dNotImplementedError, match="field_dft_device=True.*symmetry"):
        discretize(dataclasses.replace(sim, symmetry=(0, 0, 1)), n_steps=8, field_dft_device=True)
    bloch = td.BoundarySpec(x=td.Boundary.pml(num_layers=4), y=td.Boundary(minus=td.PMCBoundary(), plus=td.PECBoundary()), z=td.Boundary.bloch(0.3))
    with pytest.raises(Tidy3dNotImplementedError, match="field_dft_device=True.*Bloch"):
        discretize(dataclasses.replace(sim, boundary_spec=bloch), n_steps=8, field_dft_device=True)
    assert all(m.kind == "dft" for m in discretize(dataclasses.replace(sim, boundary_spec=bloch), n_steps=8).spec.monitors)
    spec = discretize(sim, n_steps=8, field_dft_device=True).spec
    with pytest.raises(SolverLibraryError, match="z-slab"):
        HipEngine(spec, lib=emu_lib, force_comm=True)
    i32 = lambda *v: np.asarray(v, dtype=np.int32)              # noqa: E731
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)             # noqa: E731
    comps, lo, hi, steps = i32(1, 5), i32(2, 2, 2), i32(5, 6, 6), np.asarray([1, 2], dtype=np.int64)
    nt = i32(2, 3, 3, 2, 3, 3)
    idx = np.zeros(2 * 2 * (2 + 3 + 3), dtype=np.int32)
    w = np.tile(np.asarray([1.0, 0.0], dtype=np.float32), 2 * (2 + 3 + 3))
    ph = np.ones((2, 3, 2), dtype=np.float32)                   # [n_rec][nf] complex64
    add = lambda e, ix, ww: e.lib.dll.fdtd_add_field_dft_monitor(e.handle, 2, p(comps), p(lo), p(hi), 2, p(steps), p(nt), p(ix), p(ww), 3, p(ph), p(ph))   # noqa: E731
    # the library itself refuses a z-slab handle, by message, before anything is launched
    with HipEngine(dataclasses.replace(spec, monitors=[]), lib=emu_lib, force_comm=True) as e:
        assert add(e, idx, w) < 0
        assert "fdtd_add_field_dft_monitor" in e.lib.error(e.handle) and "z-slab" in e.lib.error(e.handle)
    with HipEngine(dataclasses.replace(spec, monitors=[]), lib=emu_lib, axis_shift=0) as e:
        # the generic entry point refuses the kind and names the right one
        assert e.lib.dll.fdtd_add_monitor(e.handle, L.MON_DFT_SPARSE, 2, p(comps), p(lo), p(hi), 2, p(steps), 3, p(ph), p(ph)) < 0
        assert "fdtd_add_field_dft_monitor" in e.lib.error(e.handle)
        # a tap outside the box: index 3 along x of a box of 3 cells (second component), a negative index, a NaN weight
        for at, bad_i, bad_w in ((16, 3, 1.0), (0, -1, 1.0), (5, 0, np.nan)):
            ix, ww = idx.copy(), w.copy()
            ix[at], ww[at] = bad_i, bad_w
            assert add(e, ix, ww) < 0 and "outside the box" in e.lib.error(e.handle), (at, e.lib.error(e.handle))
        # ... but not under a zero weight; and the tables as they are are accepted
        ix = idx.copy()
        ix[17] = 99
        assert add(e, ix, w) == 0 and add(e, idx, w) == 1
        buf = (ctypes.c_int64 * 4)()
        assert e.lib.dll.fdtd_get_monitor_bytes(e.handle, 1, buf) == 0 and buf[1] == 0 and buf[2] == 8 * 3 * 2 * 18
