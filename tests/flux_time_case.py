"""The FluxTimeMonitor case shared by tests/test_emu_flux_time.py (emulator) and tests/test_gpu_flux_time.py (device), and the
checks both apply to it.

40 x 36 x 32 cells: CPML on x (4 + 4 layers of the 40), PMC / PEC on y, periodic z, a graded (CustomGrid) y axis — so the colocation
weights along y are not all 1/2 —, a lossy block, an off-centre dipole, 60 steps.  The monitors:
  px   a small x-normal plane recording every step from step 3 on (57 records): small enough for the two-step sweep to copy its
       middle-step samples out, so step pairs go through pair_record;
  py   the whole x-z cross-section, normal to the graded axis, through the CPML and around the periodic axis, every 3rd step from
       step 3 on (19 records), normal_dir "-";
  pz   a z-normal plane, every 3rd step from step 3 on;
  box  a closed box around the dipole and part of the block, every 3rd step from step 3 on (six surfaces);
  win  an x-normal plane with a start / stop window: steps 20 ... 42, every step (23 records).
57, 19 and 23 are multiples of neither 2 nor 5 (the staging rings of the wrap check).  Steps 3k + 1, 3k + 2 outside the window carry
no large record: there forced step pairs are taken."""
import dataclasses

import numpy as np

import tidy3d_amd.schema as td
from tidy3d_amd import lib as L
from tidy3d_amd.data import FieldTimeData, _diff_area, _field_container, assemble
from tidy3d_amd.discretize import discretize, flux_surfaces
from tidy3d_amd.engine import HipEngine

N_STEPS = 60
DL = 0.05
NAMES = ("px", "py", "pz", "box", "win")
EPS32 = 2.0 ** -24
HOST_BAR = 32 * EPS32           # x A_scale: <= 16 roundings of the four colocations, the products, the difference and the weights, <= 12 levels of summation
ORACLE_BAR = 4e-5               # x A_scale: twice the project's field bar of 2e-5 (the quantity is bilinear)
TWOSTEP_WORD = 5 + 64 * 4       # FDTD_OPT_TWOSTEP: five waves x four planes — forces step pairs on a grid this small


def simulation(dt=None):
    dly = tuple(0.035 + 0.03 * np.abs(np.linspace(-1, 1, 36)) ** 1.5)
    size = (32 * DL, float(np.sum(dly)), 32 * DL)
    gs = td.GridSpec(grid_x=td.UniformGrid(dl=DL), grid_y=td.CustomGrid(dl=dly), grid_z=td.UniformGrid(dl=DL))
    bspec = td.BoundarySpec(x=td.Boundary.pml(num_layers=4), y=td.Boundary(minus=td.PMCBoundary(), plus=td.PECBoundary()),
                            z=td.Boundary.periodic())
    structures = [td.Structure(geometry=td.Box(center=(0.25, 0.1, -0.1), size=(0.4, 0.35, 0.5)),
                               medium=td.Medium(permittivity=3.0, conductivity=0.02))]
    sources = [td.PointDipole(center=(-0.12, -0.07, 0.06), source_time=td.GaussianPulse(freq0=3e14, fwidth=1.5e14), polarization="Ez")]
    if dt is None:
        dt = discretize(td.Simulation(size=size, grid_spec=gs, run_time=1e-12, structures=structures, sources=sources, monitors=[],
                                      boundary_spec=bspec, shutoff=0), n_steps=4).spec.dt
    t3 = 2.5 * dt
    monitors = [
        td.FluxTimeMonitor(center=(0.18, -0.02, 0.03), size=(0, 0.2, 0.31), name="px", start=t3),
        td.FluxTimeMonitor(center=(0, 0.21, 0), size=(td.inf, 0, td.inf), name="py", interval=3, start=t3, normal_dir="-"),
        td.FluxTimeMonitor(center=(0.05, 0.0, -0.31), size=(1.2, 1.0, 0), name="pz", interval=3, start=t3),
        td.FluxTimeMonitor(center=(-0.05, -0.03, 0.02), size=(0.62, 0.55, 0.58), name="box", interval=3, start=t3),
        td.FluxTimeMonitor(center=(-0.43, 0.05, 0.0), size=(0, 0.9, 1.1), name="win", start=19.5 * dt, stop=42.5 * dt)]
    return td.Simulation(size=size, grid_spec=gs, run_time=1e-12, structures=structures, sources=sources, monitors=monitors,
                         boundary_spec=bspec, shutoff=0)


BIG_N = (520, 96, 72)           # three x tiles; with the layers below 528 x 105 x 80 cells: real step pairs with a CPML shell
BIG_STEPS = 42


def big_simulation():
    """CPML on every face of the three-tile grid, a lossy bar through the layers, three dipoles (two of them at the seam between
    x tiles at column 256), and four FluxTimeMonitors: a small x-normal plane through the seam column that the two-step sweep
    samples itself (every step), a large one through the same column, a z-normal plane in the last cell row under the z-max layers
    (inside the shell), and the x-z cross-section through all layers (every 4th step)."""
    sx, sy, sz = (n * DL for n in BIG_N)
    pulse = td.GaussianPulse(freq0=3e14, fwidth=1.5e14)
    bspec = td.BoundarySpec(x=td.Boundary(minus=td.PML(num_layers=5), plus=td.PML(num_layers=3)), y=td.Boundary.pml(num_layers=4),
                            z=td.Boundary(minus=td.PML(num_layers=3), plus=td.PML(num_layers=5)))
    bar = [td.Structure(geometry=td.Box(center=(-1.0, 0, 0), size=(td.inf, 0.8, 0.6)), medium=td.Medium(permittivity=3.0, conductivity=0.02))]
    srcs = [td.PointDipole(center=(-0.5 * sx + 255.0 * DL, 0.13, 0.07), source_time=pulse, polarization="Ey"),
            td.PointDipole(center=(-0.5 * sx + 256.5 * DL, -0.2, 0.3), source_time=pulse, polarization="Ex"),
            td.PointDipole(center=(0.3, -1.2, 1.1), source_time=pulse, polarization="Ez")]
    x_seam = -0.5 * sx + (256 - 5) * DL                  # grid line 256 of the device's x axis (five layers in front): its box holds columns 255 and 256
    mons = [td.FluxTimeMonitor(center=(x_seam, 0.1, 0.05), size=(0, 0.29, 0.29), name="seam_small"),
            td.FluxTimeMonitor(center=(x_seam, 0, 0), size=(0, 3.0, 2.4), name="seam", interval=4, start=0.0),
            td.FluxTimeMonitor(center=(0.4, 0, 0.5 * sz - 0.5 * DL), size=(9.0, 3.2, 0), name="shell", interval=4, normal_dir="-"),
            td.FluxTimeMonitor(center=(0, 0.3, 0), size=(td.inf, 0, td.inf), name="cross", interval=4)]
    return td.Simulation(size=(sx, sy, sz), grid_spec=td.GridSpec.uniform(dl=DL), run_time=1e-12, structures=bar, sources=srcs,
                         monitors=mons, boundary_spec=bspec, shutoff=0)


def discs(**kw):
    """(device-path discretization, host-path discretization) of the case"""
    sim = simulation()
    return discretize(sim, n_steps=N_STEPS, flux_time_device=True, **kw), discretize(sim, n_steps=N_STEPS, flux_time_device=False, **kw)


def with_budget(spec, records):
    """the spec with every flux-time surface's staging budget set to exactly `records` records of that surface"""
    mons = [dataclasses.replace(m, staging_bytes=records * 16 * int(np.prod(m.shape))) if m.kind == "flux_time" else m for m in spec.monitors]
    return dataclasses.replace(spec, monitors=mons)


def run_engine(spec, lib, variant=L.VARIANT_FUSED, twostep=0, n_steps=None, opts=None, axis_shift=0, **kw):
    """-> (raw results, stats) of one run on a fresh engine (twostep: the FDTD_OPT_TWOSTEP word, 0 = single steps)"""
    with HipEngine(spec, lib=lib, axis_shift=axis_shift, variant=variant, **kw) as e:
        e.set_option(L.OPT_TWOSTEP, twostep)
        if twostep:
            e.set_option(L.OPT_SHELL_PAIRS, 1)          # (whatever the cost model says of a shell this large a part of the grid)
        for k, v in (opts or {}).items():
            e.set_option(k, v)
        st = e.run(n_steps)
        return e.results(), st


def series(disc, raw):
    """name -> float32 flux series, through data.assemble (either path)"""
    sd = assemble(disc, raw)
    return {n: np.asarray(sd[n].flux.values) for n in NAMES}


def scales(disc_host, raw_host):
    """A_scale per monitor: max over the records of sum over nodes and surfaces of w (|E_t1 H_t2| + |E_t2 H_t1|), formed from the
    host path's plane records with the host path's own colocation and weights"""
    out = {}
    for plan in disc_host.plans:
        mon, tot = plan.monitor, 0.0
        t = disc_host.tmesh[plan.steps]
        for fp, (sname, box, axis, sign) in zip(plan.fields, flux_surfaces(mon)):
            class _M:
                pass
            m = _M()
            m.size, m.center, m.geometry = box.size, box.center, box
            fd = _field_container(FieldTimeData, m, disc_host.spec, fp, raw_host[fp.spec_name], "t", t, disc_host.sim.center, np.float64)
            d1, d2 = ["xyz"[a] for a in range(3) if a != axis]
            sq = lambda v: np.take(v.values, 0, axis=axis)         # noqa: E731
            a = np.abs(sq(fd["E" + d1]) * sq(fd["H" + d2])) + np.abs(sq(fd["E" + d2]) * sq(fd["H" + d1]))
            w = _diff_area(box, None, None, axis, np.asarray(fd["E" + d1].coords[d1]), np.asarray(fd["E" + d1].coords[d2]))
            tot = tot + np.tensordot(w, a, axes=([0, 1], [0, 1]))
        out[mon.name] = float(np.max(tot))
    return out


def worst_ratio(a, b, scale):
    """max over monitors and records of |a - b| / A_scale, and the monitor it occurs at"""
    worst, at = 0.0, None
    for n in NAMES:
        assert a[n].shape == b[n].shape and scale[n] > 0, n
        r = float(np.max(np.abs(a[n].astype(np.float64) - b[n].astype(np.float64))) / scale[n])
        if r >= worst:
            worst, at = r, n
    return worst, at


def same_bits(a, b):
    assert set(a) == set(b)
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and np.array_equal(x.view(np.uint32), y.view(np.uint32)), (k, np.flatnonzero(x != y)[:6])
