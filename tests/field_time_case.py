"""The FieldTimeMonitor case shared by tests/test_emu_field_time.py (emulator) and tests/test_gpu_field_time.py (device), and the
checks both apply to it: FieldTimeMonitors colocated and downsampled on the device (MonitorSpec kind "time_sparse",
csrc/fdtd_field_time.hpp) against the host path (records of the whole box, ``data._colocate_box``, ``discretize.downsample``).

The grid is the one of tests/flux_time_case.py — 40 x 36 x 32 cells: CPML on x, PMC / PEC on y with a graded y axis (the colocation
weights along y are not all 1/2), periodic z, a lossy block, an off-centre dipole, 60 steps.  The monitors, one per kind of tap table:
  vol  a volume, colocate=True, interval_space = (2, 3, 1), all six fields, every 3rd step from step 3 on (19 records): 12 primal
       nodes along x ((12 - 1) % 2 != 0: ``downsample`` appends the last index), 4 along y ((4 - 1) <= 3: nothing is dropped);
  yee  a volume, colocate=False, interval_space = (3, 1, 2), Ex and Hz: weights 1 / 0, and the two components keep different
       numbers of nodes;
  pln  a plane normal to the graded axis, off the grid lines (the zero-size axis snaps: both taps along y carry weight),
       interval_space = (1, 1, 2), across the CPML and around the whole periodic z axis (the closing samples wrap);
  top  a box that reaches the PEC wall at y max: the tap on the wall has weight 0 and an index clipped into the box;
  sml  a few cells, every step from step 3 on (57 records): small enough for the two-step sweep to copy its middle-step samples
       out, so step pairs go through pair_record; no node is dropped along x and z (its gathered array is no smaller than its box);
  win  a start / stop window: steps 20 ... 42, every step (23 records), interval_space = (1, 4, 4).
19, 57 and 23 are multiples of neither 2 nor 5 (the staging rings of the wrap check).

The large case: the 520 x 96 x 72 CPML grid of ``flux_time_case.big_simulation`` (three x tiles, 42 steps) with a volume,
interval_space = (4, 2, 2), across seam column 256, a small every-step box on the seam, and a box inside the z-max shell."""
import dataclasses

import numpy as np

import tidy3d_amd.schema as td
from tidy3d_amd.data import FieldTimeData, _field_container, assemble
from tidy3d_amd.discretize import discretize

import flux_time_case as ftc
from flux_time_case import run_engine, same_bits     # noqa: F401  (the checks' shared tools)

N_STEPS = ftc.N_STEPS
DL = ftc.DL
NAMES = ("vol", "yee", "pln", "top", "sml", "win")
N_REC = {"vol": 19, "yee": 19, "pln": 19, "top": 19, "sml": 57, "win": 23}
EPS32 = 2.0 ** -24
# |device - host| <= HOST_BAR x A, A = the largest |raw value| of the component in the record's box: three separable passes of two
# products and one add are at most 9 fp32 roundings on convex weights, one more for the host's final cast (the host interpolates in
# float64: numpy promotes float32 records times float64 weights), rounded up to a power of two
HOST_BAR = 16 * EPS32
ORACLE_BAR = 2e-5               # x the field scale: the largest |reference value| of the component in the monitor over the run
TWOSTEP_WORD = ftc.TWOSTEP_WORD
BIG_STEPS = ftc.BIG_STEPS
BIG_NAMES = ("seam_vol", "seam_small", "shell")


def simulation():
    base = ftc.simulation()
    dt = discretize(dataclasses.replace(base, monitors=[]), n_steps=4).spec.dt
    t3 = 2.5 * dt
    y_top = 0.5 * base.size[1]
    monitors = [
        td.FieldTimeMonitor(center=(0.025, -0.02, 0.03), size=(0.52, 0.09, 0.4), name="vol", interval=3, start=t3, interval_space=(2, 3, 1),
                            fields=("Ex", "Ey", "Ez", "Hx", "Hy", "Hz")),
        td.FieldTimeMonitor(center=(-0.2, 0.1, 0.1), size=(0.6, 0.3, 0.5), name="yee", interval=3, start=t3, interval_space=(3, 1, 2),
                            fields=("Ex", "Hz"), colocate=False),
        td.FieldTimeMonitor(center=(0, 0.2137, 0), size=(td.inf, 0, td.inf), name="pln", interval=3, start=t3, interval_space=(1, 1, 2),
                            fields=("Ex", "Ey", "Hz")),
        td.FieldTimeMonitor(center=(0.1, y_top - 0.1, 0.0), size=(0.3, 0.2, 0.3), name="top", interval=3, start=t3, interval_space=(1, 2, 1),
                            fields=("Ex", "Ez", "Hy")),
        td.FieldTimeMonitor(center=(0.18, -0.02, 0.03), size=(0.1, 0.07, 0.1), name="sml", start=t3, fields=("Ez", "Hx"), colocate=False),
        td.FieldTimeMonitor(center=(-0.43, 0.05, 0.0), size=(0.1, 0.9, 1.1), name="win", start=19.5 * dt, stop=42.5 * dt,
                            interval_space=(1, 4, 4), fields=("Ey", "Hx"))]
    return dataclasses.replace(base, monitors=monitors)


def big_simulation():
    base = ftc.big_simulation()
    sx, sz = ftc.BIG_N[0] * DL, ftc.BIG_N[2] * DL
    x_seam = -0.5 * sx + (256 - 5) * DL                  # grid line 256 of the device's x axis (five layers in front)
    mons = [td.FieldTimeMonitor(center=(x_seam, 0.05, 0.1), size=(2.0, 1.5, 1.2), name="seam_vol", interval=4, interval_space=(4, 2, 2),
                                fields=("Ex", "Ey", "Ez", "Hx", "Hy", "Hz")),
            td.FieldTimeMonitor(center=(x_seam, 0.1, 0.05), size=(0.1, 0.1, 0.1), name="seam_small", fields=("Ey", "Hz")),
            td.FieldTimeMonitor(center=(0.4, 0, 0.5 * sz - 1.0 * DL), size=(1.0, 0.8, 0.15), name="shell", interval=4, interval_space=(2, 2, 1),
                                fields=("Ex", "Ez", "Hy"))]
    return dataclasses.replace(base, monitors=mons)


def discs(**kw):
    """(device-path discretization, host-path discretization) of the case"""
    sim = simulation()
    return discretize(sim, n_steps=N_STEPS, field_time_device=True, **kw), discretize(sim, n_steps=N_STEPS, field_time_device=False, **kw)


def with_budget(spec, records):
    """the spec with every sparse field-time monitor's staging budget set to exactly `records` records of that monitor"""
    mons = [dataclasses.replace(m, staging_bytes=records * 4 * len(m.comps) * int(np.prod(m.shape))) if m.kind == "time_sparse" else m
            for m in spec.monitors]
    return dataclasses.replace(spec, monitors=mons)


def gathered_bytes(m):
    """what the library must report for the gathered array of the sparse monitor spec `m`"""
    return 4 * len(m.steps) * sum(int(np.prod(t)) for t in m.targets)


def fields(disc, raw, names=NAMES, dtype=np.float32):
    """(monitor, field) -> values [nx_t, ny_t, nz_t, n_rec] as data.assemble builds them (either path: ``_field_container`` is
    what assemble calls for a FieldTimeMonitor).  dtype float64: an fp64 oracle's records stay float64 all the way."""
    if dtype == np.float32:
        sd = assemble(disc, raw)
    out = {}
    for plan in disc.plans:
        mon, fp = plan.monitor, plan.fields[0]
        if mon.name not in names:
            continue
        fd = sd[mon.name] if dtype == np.float32 else _field_container(FieldTimeData, mon, disc.spec, fp, raw[fp.spec_name], "t",
                                                                       disc.tmesh[plan.steps], disc.sim.center, dtype)
        for f in fp.fields:
            out[(mon.name, f)] = np.asarray(getattr(fd, f).values)
    return out


def box_scales(disc_host, raw_host, names=NAMES):
    """(monitor, field) -> A [n_rec]: the largest |raw value| of the component in each record's box on the host path"""
    out = {}
    for plan in disc_host.plans:
        if plan.monitor.name in names:
            fp = plan.fields[0]
            for ic, f in enumerate(fp.fields):
                out[(plan.monitor.name, f)] = np.abs(raw_host[fp.spec_name][:, ic].astype(np.float64)).reshape(len(plan.steps), -1).max(axis=1)
    return out


def worst_host_ratio(dev, host, scale):
    """max over monitors, fields, records and nodes of |device - host| / A (a record whose box is all zero must agree exactly),
    where it occurs, and per (monitor, field) the share of bit-identical values"""
    worst, at, same = 0.0, None, {}
    for k in host:
        a, b = dev[k], host[k]
        assert a.dtype == np.float32 and b.dtype == np.float32 and a.shape == b.shape and b.shape[-1] == len(scale[k]), k
        d = np.abs(a.astype(np.float64) - b.astype(np.float64)).reshape(-1, b.shape[-1]).max(axis=0)
        A = scale[k]
        assert not d[A == 0].any(), k
        r = float(np.max(np.where(A > 0, d / np.where(A > 0, A, 1.0), 0.0)))
        if r >= worst:
            worst, at = r, k
        same[k] = float(np.mean(a.view(np.uint32) == b.view(np.uint32)))
    return worst, at, same


def worst_oracle_ratio(dev, ref):
    worst, at = 0.0, None
    for k in ref:
        s = float(np.abs(ref[k]).max())
        assert s > 0 and dev[k].shape == ref[k].shape, k
        r = float(np.abs(dev[k].astype(np.float64) - ref[k]).max()) / s
        if r >= worst:
            worst, at = r, k
    return worst, at
