"""The projection-monitor case shared by tests/test_emu_projection_dft.py (emulator) and tests/test_gpu_projection_dft.py (device), and
the checks both apply to it: the surfaces of field projection monitors accumulated on their sampling lattice only, on the device
(MonitorSpec kind "dft_lattice", csrc/fdtd_lattice_dft.hpp), against the host path (accumulators over the whole padded box,
``data._colocate_box``, ``data.interp_axis``).

The grid is the one of tests/flux_time_case.py — 40 x 36 x 32 cells: CPML on x, PMC / PEC on y with a graded y axis (the taps along y
vary from node to node), periodic z, a lossy block, an off-centre dipole, 60 steps.  Three frequencies.  The monitors:
  box   a closed FieldProjectionAngleMonitor around the dipole and part of the block: six surfaces, all three orientations — on the
        two surfaces normal to x the lanes of the kernel run along y (nt[.][0] == 1);
  cart  a FieldProjectionCartesianMonitor plane normal to z with window_size = (0.3, 0.2) and far_field_approx=False;
  ksp   a FieldProjectionKSpaceMonitor plane normal to the graded axis, td.inf wide: past the domain on x (the lattice is clipped to
        the domain, its ends lie in the CPML) and around the whole periodic z axis (the closing samples wrap);
  med   a plane normal to x with a projection medium of index 3: its lattice (0.027 um) is finer than the grid (0.035 - 0.065 um
        along y, 0.05 um along z) — several lattice points per cell, repeated indices;
  top   a plane normal to y inside the last cell under the PEC wall at y max: the padded box reaches the wall, so the colocation
        of Ex and Ez along y takes its upper sample — zero — on the wall itself (the "wall" closing: a slot of weight 0).

The large case: the 520 x 96 x 72 CPML grid of ``flux_time_case.big_simulation`` (three x tiles, 42 steps) with a plane normal to z
across seam column 256, a plane normal to x (both with a projection medium of index 2: more than 64 lattice points along the
kernel's lane axis — x on the first, y on the second — so more than one workgroup along it), and a plane normal to y reaching into the
z-max CPML."""
import dataclasses

import numpy as np

import tidy3d_amd.schema as td
from tidy3d_amd.data import FieldData, _field_container, interp_axis
from tidy3d_amd.discretize import discretize, flux_surfaces
from tidy3d_amd.projection import surface_lattice

import flux_time_case as ftc
from flux_time_case import run_engine, same_bits     # noqa: F401  (the checks' shared tools)

N_STEPS = ftc.N_STEPS
DL = ftc.DL
NAMES = ("box", "cart", "ksp", "med", "top")
FREQS = (2.4e14, 3.0e14, 3.7e14)
EPS32 = 2.0 ** -24
# |device - host| <= HOST_BAR x A, A = the largest |accumulator| of the component and frequency over the surface's box in the host run.
# The rule (that of field_dft_case.HOST_BAR): the worst figure measured on the emulator (MEASURED_HOST below, printed by the tests),
# times 4, rounded up to a power of two x 2^-24.  The host colocates and resamples the fp32 accumulators in float64; the device
# forms every sample in fp32 — three passes of up to four products and three adds — and accumulates the result: the two differ by
# rounding order only.
MEASURED_HOST = (2.620, ("box::z-", "Ey"))          # x 2^-24 and where, on the emulator: x 4 = 10.5 -> 16
HOST_BAR = 16 * EPS32
ORACLE_BAR = 2e-5               # x the largest |reference value| of the component on the lattices of the monitor's surfaces
# the six spherical components of web.run(projection_device=True) against False, relative to the largest |component| of the
# monitor and frequency: the same rule (MEASURED_END x 4, rounded up to a power of two x 2^-24)
MEASURED_END = (2.817, ("cart", "Etheta"))          # x 2^-24 and where, on the emulator (the exact projection of `cart`): x 4 = 11.3 -> 16
END_BAR = 16 * EPS32
TWOSTEP_WORD = ftc.TWOSTEP_WORD
BIG_STEPS = ftc.BIG_STEPS
BIG_NAMES = ("seam_z", "plane_x", "shell")


def simulation():
    base = ftc.simulation()
    y_top = 0.5 * base.size[1]
    dy_last = float(base.grid_spec.grid_y.dl[-1])
    monitors = [
        td.FieldProjectionAngleMonitor(center=(-0.05, -0.03, 0.02), size=(0.62, 0.55, 0.58), name="box", freqs=FREQS,
                                       theta=(0.3, 1.1, 2.0), phi=(0.0, 0.9)),
        td.FieldProjectionCartesianMonitor(center=(0.05, 0.0, -0.31), size=(1.2, 1.0, 0), name="cart", freqs=FREQS, normal_dir="-",
                                           x=(-1.0, 0.5), y=(0.3,), proj_distance=4.0, proj_axis=2, window_size=(0.3, 0.2),
                                           far_field_approx=False),
        td.FieldProjectionKSpaceMonitor(center=(0, 0.2137, 0), size=(td.inf, 0, td.inf), name="ksp", freqs=FREQS, normal_dir="+",
                                        ux=(-0.3, 0.2), uy=(0.0, 0.4), proj_axis=1),
        td.FieldProjectionAngleMonitor(center=(0.18, -0.02, 0.03), size=(0, 0.5, 0.6), name="med", freqs=FREQS, normal_dir="+",
                                       theta=(1.2, 1.6), phi=(0.0, 0.4), medium=td.Medium(permittivity=9.0)),
        td.FieldProjectionAngleMonitor(center=(0.1, y_top - 0.4 * dy_last, 0.0), size=(0.9, 0, 0.7), name="top", freqs=FREQS,
                                       normal_dir="+", theta=(0.8, 1.4), phi=(1.2, 1.8))]
    return dataclasses.replace(base, monitors=monitors)


def big_simulation():
    base = ftc.big_simulation()
    sx, sz = ftc.BIG_N[0] * DL, ftc.BIG_N[2] * DL
    x_seam = -0.5 * sx + (256 - 5) * DL                  # grid line 256 of the device's x axis (five layers in front)
    mon = lambda **kw: td.FieldProjectionAngleMonitor(freqs=FREQS, theta=(0.4, 1.3), phi=(0.0, 1.0), **kw)          # noqa: E731
    n2 = td.Medium(permittivity=4.0)                     # (half the lattice spacing: more than 64 lattice points along a row)
    mons = [mon(center=(x_seam, 0.05, 0.4), size=(4.0, 1.5, 0), name="seam_z", normal_dir="+", medium=n2),
            mon(center=(x_seam + 0.52, 0.1, 0.05), size=(0, 4.0, 1.9), name="plane_x", normal_dir="+", medium=n2),
            mon(center=(0.4, 0.62, 0.5 * sz - 0.5), size=(3.0, 0, 1.3), name="shell", normal_dir="+")]
    return dataclasses.replace(base, monitors=mons)


def discs(sim=None, steps=N_STEPS):
    """(device-path discretization, host-path discretization) of the case"""
    sim = simulation() if sim is None else sim
    return discretize(sim, n_steps=steps, projection_device=True), discretize(sim, n_steps=steps, projection_device=False)


def lattice_bytes(disc, name):
    """what the library must report for the accumulators of the monitor `name` on the device path: nf x lattice nodes x 8 B"""
    return sum(8 * len(m.freqs) * sum(int(np.prod(t)) for t in m.targets) for m in disc.spec.monitors if m.name.split("::")[0] == name)


def surfaces(disc, names=NAMES):
    """(plan, surface index, FieldPlan, box, axis) of every surface of the case"""
    for plan in disc.plans:
        if plan.monitor.name in names:
            for i, (fp, (sname, box, axis, sign)) in enumerate(zip(plan.fields, flux_surfaces(plan.monitor))):
                yield plan, i, fp, box, axis


def lattice_values(disc, raw, names=NAMES, dtype=np.complex64):
    """(surface, field) -> accumulated values [n_u, n_v, nf] on the sampling lattice, before the source normalisation.  Device path
    (two-dimensional raw): as the library returns them.  Host path, and an fp64 oracle's accumulators (dtype complex128): the whole
    box colocated (``_field_container``) and resampled (``interp_axis``) by the float64 host code projection._surface_currents runs."""
    out = {}
    for plan, i, fp, box, axis in surfaces(disc, names):
        mon, r = plan.monitor, raw[fp.spec_name]
        pts = surface_lattice(disc.sim, mon, box, axis)
        n = [len(p) for p in pts]
        if np.ndim(r) == 2:
            assert plan.lattices is not None and all(np.array_equal(p, q) for p, q in zip(plan.lattices[i], pts)), fp.spec_name
            assert r.shape == (len(FREQS), 4 * int(np.prod(n))) and r.dtype == np.complex64, (fp.spec_name, r.shape)
            for ic, f in enumerate(fp.fields):
                blk = r[:, ic * int(np.prod(n)):(ic + 1) * int(np.prod(n))].reshape(len(FREQS), n[2], n[1], n[0])
                out[(fp.spec_name, f)] = np.take(np.transpose(blk, (3, 2, 1, 0)), 0, axis=axis)
            continue

        class _M:
            pass
        m = _M()
        m.size, m.center, m.geometry, m.name = box.size, box.center, box, fp.spec_name
        fd = _field_container(FieldData, m, disc.spec, fp, r, "f", np.asarray(FREQS), disc.sim.center, np.complex128)
        for f in fp.fields:
            arr = np.asarray(fd[f].values)
            for a in range(3):
                if a != axis:
                    arr = interp_axis(arr, np.asarray(fd[f].coords["xyz"[a]]), pts[a], axis=a)
            out[(fp.spec_name, f)] = np.take(arr, 0, axis=axis).astype(dtype)
    return out


def box_scales(disc_host, raw_host, names=NAMES):
    """(surface, field) -> A [nf]: the largest |accumulator| of the component over the surface's whole box, per frequency, host path"""
    out = {}
    for plan, i, fp, box, axis in surfaces(disc_host, names):
        for ic, f in enumerate(fp.fields):
            acc = raw_host[fp.spec_name][:, ic]
            out[(fp.spec_name, f)] = np.abs(acc.astype(np.complex128)).reshape(acc.shape[0], -1).max(axis=1)
    return out


def worst_host_ratio(dev, host, scale):
    """max over surfaces, fields, frequencies and lattice points of |device - host| / A, and where it occurs"""
    worst, at = 0.0, None
    assert set(dev) == set(host)
    for k in host:
        a, b = dev[k], host[k]
        assert a.dtype == np.complex64 and a.shape == b.shape and b.shape[-1] == len(scale[k]), (k, a.shape, b.shape)
        d = np.abs(a.astype(np.complex128) - b.astype(np.complex128)).reshape(-1, b.shape[-1]).max(axis=0)
        A = scale[k]
        assert (A > 0).all(), k
        r = float(np.max(d / A))
        if r >= worst:
            worst, at = r, k
    return worst, at


def worst_oracle_ratio(dev, ref):
    """max over surfaces and fields of |dev - ref| / the largest |reference value| of the component in the monitor — over all the
    surfaces of the monitor that carry the component, the project's field scale (field_dft_case.worst_oracle_ratio): the fp32
    error of a sample follows the largest field the solver carries near it, not the field on the far side of a closed box"""
    scale = {}
    for (sname, f), v in ref.items():
        k = (sname.split("::")[0], f)
        scale[k] = max(scale.get(k, 0.0), float(np.abs(v).max()))
    worst, at = 0.0, None
    for k in ref:
        s = scale[(k[0].split("::")[0], k[1])]
        assert s > 0 and dev[k].shape == ref[k].shape, k
        r = float(np.abs(dev[k].astype(np.complex128) - ref[k]).max()) / s
        if r >= worst:
            worst, at = r, k
    return worst, at


SPHERICAL = ("Er", "Etheta", "Ephi", "Hr", "Htheta", "Hphi")


def worst_end_ratio(sd_dev, sd_host, names=NAMES):
    """max over monitors, the six spherical components and frequencies of |device - host| / S, and where it occurs.  S = the largest
    |component| of the monitor at that frequency on the host path, taken over the three E components for an E component and over
    the three H components for an H component (Er and Hr are zero in the far-field approximation and much smaller than the others
    elsewhere: a scale of their own would measure nothing).  The containers must agree in type, coordinates, dims and dtype."""
    worst, at = 0.0, None
    for n in names:
        a, b = sd_dev[n], sd_host[n]
        assert type(a) is type(b), n
        fa = getattr(b, "Er").dims.index("f")
        other = tuple(i for i in range(np.asarray(b.Er.values).ndim) if i != fa)
        scale = {g: np.max([np.nan_to_num(np.abs(np.asarray(getattr(b, c).values))).max(axis=other) for c in SPHERICAL if c[0] == g], axis=0)
                 for g in "EH"}
        for c in SPHERICAL:
            xa, xb = getattr(a, c), getattr(b, c)
            va, vb = np.asarray(xa.values), np.asarray(xb.values)
            assert va.dtype == vb.dtype and va.shape == vb.shape and xa.dims == xb.dims and list(xa.coords) == list(xb.coords), (n, c)
            assert all(np.array_equal(np.asarray(xa.coords[k]), np.asarray(xb.coords[k])) for k in xa.coords), (n, c)
            assert np.array_equal(np.isnan(va), np.isnan(vb)), (n, c)          # (evanescent directions of a k-space monitor)
            assert (scale[c[0]] > 0).all(), (n, c)
            r = float(np.max(np.nan_to_num(np.abs(va - vb)).max(axis=other) / scale[c[0]]))
            if r >= worst:
                worst, at = r, (n, c)
    return worst, at
