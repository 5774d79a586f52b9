"""FullyAnisotropicMedium together with Bloch boundaries.  The off-diagonal coupling lists (spec.AnisoSet, csrc/fdtd_aniso.hpp) reach
across a periodic face to the real node on the far side; under a Bloch face that node stands for exp(+-i phi) E, so the coupling
mixes the Re and Im solvers (fdtd_add_aniso_bloch wrap codes, fdtd_run_bloch).  Pins on the HIP-on-CPU emulator:

  - a body clear of the wraps against the oracle (the index mapping onto the ghost-cell device layout and the schedule);
  - a body cut by the x and y wraps against the same cell translated by whole cells so that the body lies inside: the fields
    agree after the Bloch phase of the cells that crossed a wrap (the phase in the kernel; no oracle needed);
  - the 4 x 4 transfer-matrix reference the device's physics pin (tests/test_gpu_aniso_bloch.py) uses, against the Airy formulas;
  - what is still refused.
"""
import ctypes

import numpy as np
import pytest

import tidy3d_amd.schema as td
from tidy3d_amd import lib as L
from tidy3d_amd.constants import C_0
from tidy3d_amd.discretize import discretize
from tidy3d_amd.exceptions import Tidy3dNotImplementedError

from oracle.fdtd_numpy import OracleFdtd

DL = 0.05
PULSE = td.GaussianPulse(freq0=3e14, fwidth=1.5e14)
PHASES = (0.31, -0.17, 0.45)


def rot(axis, angle):
    c, s = np.cos(angle), np.sin(angle)
    m = {2: [[c, -s, 0], [s, c, 0], [0, 0, 1]], 1: [[c, 0, s], [0, 1, 0], [-s, 0, c]], 0: [[1, 0, 0], [0, c, -s], [0, s, c]]}[axis]
    return np.array(m)


BIAXIAL = td.FullyAnisotropicMedium.from_diagonal(2.0, 5.0, 3.2, rot(2, 0.7) @ rot(1, 0.4))


def clear_case(z="bloch", N=(18, 14, 12)):
    """A rotated biaxial sphere and a lossy block well inside a Bloch cell (x, y and z, or x and y with CPML z), a dipole, a time
    and a DFT monitor: no coupling row crosses a wrap."""
    from cases import _sim
    structures = [td.Structure(geometry=td.Sphere(center=(0.03, 0.01, 0.0), radius=0.2), medium=BIAXIAL),
                  td.Structure(geometry=td.Box(center=(-0.3, 0.18, 0), size=(0.1, 0.12, 0.2)),
                               medium=td.Medium(permittivity=2.5, conductivity=0.02))]
    bz = td.Boundary.bloch(PHASES[2]) if z == "bloch" else td.Boundary.pml(num_layers=3)
    bspec = td.BoundarySpec(x=td.Boundary.bloch(PHASES[0]), y=td.Boundary.bloch(PHASES[1]), z=bz)
    return _sim(N, bspec, structures)


def wrapped_cell(center=(0.0, 0.0, 0.0), N=(18, 14, 10), bloch=(0.23, -0.31), run_time=1e-12, lossless=False):
    """A uniform-grid Bloch cell (x, y; PEC z walls) of period N cells with a biaxial sphere on the lattice point at the cell's
    (+x, +y) corner (its images on the other three corners complete it): cut by the x wrap, the y wrap and both at once.
    ``center`` moves the cell's window by whole cells; the lossy box and the dipoles lie where both windows hold them."""
    size = tuple(n * DL for n in N)
    structures = [td.Structure(geometry=td.Sphere(center=(sx * 0.5 * size[0], sy * 0.5 * size[1], 0.0), radius=0.18), medium=BIAXIAL)
                  for sx in (-1, 1) for sy in (-1, 1)]
    if not lossless:
        structures.append(td.Structure(geometry=td.Box(center=(0.25, 0.05, 0.0), size=(0.11, 0.07, 0.19)),
                                       medium=td.Medium(permittivity=2.5, conductivity=0.02)))
    return td.Simulation(size=size, center=center, grid_spec=td.GridSpec.uniform(dl=DL), run_time=run_time, subpixel=False,
                         structures=structures, shutoff=0,
                         sources=[td.PointDipole(center=(0.12, 0.07, 0.03), source_time=PULSE, polarization="Ez"),
                                  td.PointDipole(center=(0.07, 0.2, -0.06), source_time=PULSE, polarization="Hx")],
                         boundary_spec=td.BoundarySpec(x=td.Boundary.bloch(bloch[0]), y=td.Boundary.bloch(bloch[1]),
                                                       z=td.Boundary.pec()))


def translated_fields(lib, variant, n_steps=150, N=(18, 14, 10)):
    """Run the corner cell A and the same cell with its window moved by half a period along x and y (B: the sphere in the middle);
    map B's fields back onto A's cells, exp(-i phi) on the cells that lie one period back.  Returns (A's fields, B's mapped)."""
    from tidy3d_amd.engine import HipEngine
    sx, sy = N[0] // 2, N[1] // 2
    out = []
    for center in ((0.0, 0.0, 0.0), (sx * DL, sy * DL, 0.0)):
        disc = discretize(wrapped_cell(center=center, N=N), n_steps=n_steps)
        with HipEngine(disc.spec, lib=lib, variant=variant) as e:
            e.run()
            out.append(([e.get_field(c) for c in range(6)], disc.spec))
    (fa, spec_a), (fb, spec_b) = out
    # A's sphere is cut by both wraps (rows with slots that cross x, y and both); B's lies inside
    for spec, crossing in ((spec_a, True), (spec_b, False)):
        w = np.concatenate([np.abs(st.nbr_wrap[st.g != 0]).reshape(-1, 3) for st in spec.aniso])
        assert w[:, :2].any(axis=1).any() == crossing
        if crossing:
            assert w[:, 0].any() and w[:, 1].any() and (w[:, 0] & w[:, 1]).any()
    phx, phy = spec_a.bloch[0], spec_a.bloch[1]
    mapped = []
    for f in fb:
        g = np.roll(f, (sy, sx), axis=(1, 2))                 # A's cell i holds B's cell i - s
        g[:, :, :sx] *= np.exp(-1j * phx)                      # ... which lies one period back for i < s
        g[:, :sy, :] *= np.exp(-1j * phy)
        mapped.append(g)
    return fa, mapped


def assert_translation(fa, mapped, tol=1e-5):
    for grp in ((0, 1, 2), (3, 4, 5)):
        num = np.sqrt(sum(np.linalg.norm(fa[c] - mapped[c]) ** 2 for c in grp))
        den = np.sqrt(sum(np.linalg.norm(fa[c]) ** 2 for c in grp))
        assert den > 0 and num / den < tol, (grp, num / den)


def compare_with_oracle(lib, variant, z, n_steps=80, tol=2e-5):
    from cases import rel_err
    from tidy3d_amd.engine import HipEngine
    disc = discretize(clear_case(z), n_steps=n_steps)
    spec = disc.spec
    assert spec.bloch is not None and len(spec.aniso) == 3
    for st in spec.aniso:                                  # no coupling row crosses a wrap
        assert not np.abs(st.nbr_wrap[st.g != 0]).any()
    o = OracleFdtd(spec)
    ref = o.run()
    with HipEngine(spec, lib=lib, variant=variant) as e:
        e.run()
        got = e.results()
        f = [e.get_field(c) for c in range(6)]
    for k in ref:
        assert rel_err(got[k], ref[k]) < tol, k
    en = np.sqrt(sum(np.linalg.norm(x) ** 2 for x in o.E))
    hn = np.sqrt(sum(np.linalg.norm(x) ** 2 for x in o.H))
    assert max(float(np.linalg.norm(f[c] - o.E[c]) / en) for c in range(3)) < tol
    assert max(float(np.linalg.norm(f[3 + c] - o.H[c]) / hn) for c in range(3)) < tol


def compare_wrapped_with_oracle(lib, variant, n_steps=100, tol=2e-5):
    """``compare_with_oracle`` for the corner cell, a time and a DFT monitor added: rows that cross the x wrap, the y wrap and both.  The
    oracle rotates the curl it recovers through such a slot by the Bloch factor (tests/test_aniso_nodes.py pins that factor)."""
    import dataclasses
    from cases import rel_err
    from tidy3d_amd.engine import HipEngine
    monitors = [td.FieldTimeMonitor(center=(0.3, 0.25, 0.0), size=(0.25, 0.15, 0.1), name="t", colocate=False, interval=7),
                td.FieldMonitor(center=(0, 0, 0), size=(0.8, 0.6, 0), freqs=[2.5e14, 3e14], name="f")]
    spec = discretize(dataclasses.replace(wrapped_cell(), monitors=monitors), n_steps=n_steps).spec
    w = np.concatenate([np.abs(st.nbr_wrap[st.g != 0]).reshape(-1, 3) for st in spec.aniso])
    assert w[:, 0].any() and w[:, 1].any() and (w[:, 0] & w[:, 1]).any()
    o = OracleFdtd(spec)
    ref = o.run()
    with HipEngine(spec, lib=lib, variant=variant) as e:
        e.run()
        got = e.results()
        f = [e.get_field(c) for c in range(6)]
    assert set(ref) == {"t", "f"}
    for k in ref:
        assert rel_err(got[k], ref[k]) < tol, k
    en = np.sqrt(sum(np.linalg.norm(x) ** 2 for x in o.E))
    hn = np.sqrt(sum(np.linalg.norm(x) ** 2 for x in o.H))
    assert max(float(np.linalg.norm(f[c] - o.E[c]) / en) for c in range(3)) < tol
    assert max(float(np.linalg.norm(f[3 + c] - o.H[c]) / hn) for c in range(3)) < tol


def test_wrap_signs_of_the_coupling_lists():
    """_aniso_sets records the period each slot crossed: +1 beyond the upper face, -1 beyond the lower one, on periodic axes
    only; wrapping the unwrapped neighbour index back into the grid gives nbr_ijk."""
    spec = discretize(wrapped_cell(), n_steps=2).spec
    shape = np.array(spec.shape)
    seen = set()
    for st in spec.aniso:
        a = st.comp
        for slot in range(8):
            b = st.nbr_comp[slot]
            da, db = (0, 1, 0, 1)[slot % 4], (-1, -1, 0, 0)[slot % 4]
            raw = st.ijk.copy()
            raw[:, a] += da
            raw[:, b] += db
            w = st.nbr_wrap[:, slot].astype(np.int64)
            assert np.array_equal(raw, st.nbr_ijk[:, slot] + w * shape[None, :])
            assert not w[:, 2].any()                       # z: PEC walls, nothing wraps
            seen |= {tuple(r) for r in np.unique(w, axis=0)}
    assert {(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (1, -1, 0), (-1, 1, 0)} <= seen


@pytest.mark.parametrize("z", ["bloch", "pml"])
@pytest.mark.parametrize("variant", ["fused", "two_pass"])
def test_body_clear_of_the_wraps_matches_the_oracle(variant, z, emu_lib):
    compare_with_oracle(emu_lib, L.VARIANT_FUSED if variant == "fused" else L.VARIANT_ZMARCH, z)


@pytest.mark.parametrize("variant", ["fused", "two_pass"])
def test_body_across_the_wraps_is_a_translation(variant, emu_lib):
    fa, mapped = translated_fields(emu_lib, L.VARIANT_FUSED if variant == "fused" else L.VARIANT_ZMARCH)
    assert_translation(fa, mapped)


@pytest.mark.parametrize("variant", ["fused", "two_pass"])
def test_body_across_the_wraps_matches_the_oracle(variant, emu_lib):
    compare_wrapped_with_oracle(emu_lib, L.VARIANT_FUSED if variant == "fused" else L.VARIANT_ZMARCH)


def test_bad_wrap_codes_are_refused(emu_lib):
    from tidy3d_amd.engine import HipEngine
    spec = discretize(wrapped_cell(), n_steps=2).spec
    with HipEngine(spec, lib=emu_lib) as e:
        d = e.lib.dll
        cells = np.zeros(1, np.uint32)
        nbr = np.zeros(8, np.uint32)
        w = np.zeros(8, np.float32)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)    # noqa: E731
        for bad in (3, 0b1100, 0b110000, 64):
            wrap = np.zeros(8, np.uint8)
            wrap[5] = bad
            assert d.fdtd_add_aniso_bloch(e.handle, 1, 1, p(cells), p(nbr), p(w), p(w), p(wrap)) < 0
            assert "wrap code" in e.lib.error(e.handle)
        assert d.fdtd_add_aniso_bloch(e.handle, 1, 1, p(cells), p(nbr), p(w), p(w), None) < 0


def test_what_is_still_refused(emu_lib):
    """Aniso + Bloch on z-slabs keeps its error (the engine raises before the library would)."""
    from tidy3d_amd.engine import HipEngine
    disc = discretize(clear_case("bloch", N=(12, 10, 8)), n_steps=2)
    with pytest.raises(Tidy3dNotImplementedError, match="z-slab"):
        HipEngine(disc.spec, lib=emu_lib, force_comm=True)


# ---------------------------------------------------------------------------------------------------------------------------------
# 4 x 4 transfer matrix (Berreman) of a homogeneous anisotropic slab in vacuum: the reference of the device's physics pin


def _delta(eps, kx, ky):
    """d/dz (Ex, Ey, hx, hy) = i k0 Delta (...), h = Z0 H, fields ~ exp(i (k0 kx x + k0 ky y) - i w t) (kx, ky in units of k0)."""
    D = np.zeros((4, 4), complex)
    for col in range(4):
        ex, ey, hx, hy = np.eye(4)[col]
        ez = (ky * hx - kx * hy - eps[2, 0] * ex - eps[2, 1] * ey) / eps[2, 2]
        hz = kx * ey - ky * ex
        ev = np.array([ex, ey, ez])
        D[:, col] = [hy + kx * ez, ky * ez - hx, kx * hz - eps[1] @ ev, ky * hz + eps[0] @ ev]
    return D


def vacuum_modes(kx, ky, sign):
    """(s, p) plane waves of vacuum travelling along +z (sign = 1) or -z: their E vectors [2, 3] and (Ex, Ey, hx, hy) [4, 2]."""
    kz = sign * np.sqrt(1 - kx ** 2 - ky ** 2 + 0j)
    k = np.array([kx, ky, kz])
    kt = np.hypot(kx, ky)
    s = np.array([-ky, kx, 0.0]) / kt if kt > 0 else np.array([0.0, 1.0, 0.0])
    p = np.cross(s, k)
    E = np.stack([s, p])
    psi = np.array([[e[0], e[1], np.cross(k, e)[0], np.cross(k, e)[1]] for e in E]).T
    return E, psi


def berreman_slab(eps, d_um, freqs, kpar, inc_pol):
    """Amplitudes of the plane wave of fixed in-plane wavevector ``kpar`` (rad/um) and unit amplitude along ``inc_pol`` ("s" or "p")
    that a slab of thickness d_um (relative permittivity tensor eps) in vacuum transmits / reflects: t, r [nf, 2] in the (s, p)
    basis of vacuum_modes, each relative to the incident wave at the slab's entry face (t taken at the exit face)."""
    from scipy.linalg import expm
    t_out, r_out = [], []
    for f in freqs:
        k0 = 2 * np.pi * f / C_0                           # rad/um (C_0 in um/s)
        kx, ky = kpar[0] / k0, kpar[1] / k0
        _, fwd = vacuum_modes(kx, ky, 1)
        _, bwd = vacuum_modes(kx, ky, -1)
        M = expm(1j * k0 * d_um * _delta(np.asarray(eps, complex), kx, ky))
        a = np.array([1.0, 0.0]) if inc_pol == "s" else np.array([0.0, 1.0])
        # M (fwd a + bwd r) = fwd t
        A = np.concatenate([M @ bwd, -fwd], axis=1)
        x = np.linalg.solve(A, -M @ fwd @ a)
        r_out.append(x[:2])
        t_out.append(x[2:])
    return np.array(t_out), np.array(r_out)


def test_transfer_matrix_reference_against_airy():
    """The reference of the physics pin: an isotropic slab gives the Airy coefficients of s and p light at oblique incidence,
    lossless slabs conserve power, and a rotated uniaxial one converts polarisation."""
    n, d = 1.7, 0.6
    freqs = np.linspace(1.7e14, 2.3e14, 7)
    theta, phi = 0.5, 0.4
    k0c = 2 * np.pi * 2e14 / C_0
    kpar = k0c * np.sin(theta) * np.array([np.cos(phi), np.sin(phi)])
    for pol in ("s", "p"):
        t, r = berreman_slab(n ** 2 * np.eye(3), d, freqs, kpar, pol)
        k0 = 2 * np.pi * freqs / C_0
        st = np.hypot(*kpar) / k0
        c1, c2 = np.sqrt(1 - st ** 2), np.sqrt(1 - (st / n) ** 2)
        r12 = (c1 - n * c2) / (c1 + n * c2) if pol == "s" else (n * c1 - c2) / (n * c1 + c2)
        beta = k0 * n * c2 * d
        T = (1 - r12 ** 2) ** 2 / np.abs(1 - r12 ** 2 * np.exp(2j * beta)) ** 2
        i, j = (0, 1) if pol == "s" else (1, 0)
        assert np.allclose(np.abs(t[:, i]) ** 2, T, rtol=1e-10, atol=1e-12)
        assert np.abs(t[:, j]).max() < 1e-12 and np.abs(r[:, j]).max() < 1e-12
        assert np.allclose(np.sum(np.abs(t) ** 2 + np.abs(r) ** 2, axis=1), 1.0, atol=1e-12)
    eps = rot(2, 0.6) @ rot(1, 0.5) @ np.diag([1.8 ** 2, 1.5 ** 2, 1.5 ** 2]) @ (rot(2, 0.6) @ rot(1, 0.5)).T
    t, r = berreman_slab(eps, d, freqs, kpar, "p")
    assert np.allclose(np.sum(np.abs(t) ** 2 + np.abs(r) ** 2, axis=1), 1.0, atol=1e-12)
    assert np.abs(t[:, 0]).min() > 0.05
