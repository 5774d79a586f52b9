"""FullyAnisotropicMedium together with Bloch boundaries on the device (the emulator's pins are in tests/test_aniso_bloch.py):

  (a) a body clear of the wraps against the oracle, fused sweep and two-pass kernels;
  (b) a body cut by the x and y wraps against the same cell translated by whole cells (the phase of the coupling across a wrap),
      and against the oracle, which carries that phase itself;
  (c) physics: an oblique plane wave through a rotated uniaxial slab that fills the period, against the 4 x 4 transfer matrix —
      co- and cross-polarised transmission and the reflected / transmitted power; the bar is set by the same set-up with an
      isotropic slab (the discretisation's own error: staircased faces, numerical dispersion);
  (d) a closed, lossless Bloch cell with a body across both wraps stays bounded for 20k steps (a coupling that is not Hermitian
      grows here).
"""
import numpy as np
import pytest

import tidy3d_amd.schema as td
from tidy3d_amd import lib as L
from tidy3d_amd.data import assemble
from tidy3d_amd.discretize import discretize
from tidy3d_amd.engine import HipEngine

from test_aniso_bloch import (assert_translation, berreman_slab, compare_with_oracle, compare_wrapped_with_oracle, rot, translated_fields, vacuum_modes,
                              wrapped_cell)

pytestmark = pytest.mark.gpu

VARIANTS = {"fused": L.VARIANT_FUSED, "two_pass": L.VARIANT_ZMARCH}


@pytest.mark.parametrize("z", ["bloch", "pml"])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_body_clear_of_the_wraps_matches_the_oracle(variant, z, hip_lib):
    compare_with_oracle(hip_lib, VARIANTS[variant], z, n_steps=120)


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_body_across_the_wraps_is_a_translation(variant, hip_lib):
    fa, mapped = translated_fields(hip_lib, VARIANTS[variant], n_steps=200)
    assert_translation(fa, mapped)


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_body_across_the_wraps_matches_the_oracle(variant, hip_lib):
    compare_wrapped_with_oracle(hip_lib, VARIANTS[variant], n_steps=120)


# ------------------------------------------------------------------------------------------------------------- (c) physics
SLAB_D = 0.6
FREQS = np.linspace(1.75e14, 2.25e14, 7)
THETA, PHI = 0.45, 0.5
N_O, N_E = 1.5, 1.8
AXES = rot(2, 0.6) @ rot(1, 0.5)          # the optic axis (the first column) neither in nor normal to the plane of incidence
N_ISO = 1.7


def slab_run(lib, medium):
    """Oblique p-polarised PlaneWave (Bloch x / y from the source, CPML z) onto a slab that fills the period; flux planes either
    side, a field probe behind the slab.  Returns (flux in front [nf], flux behind [nf], probe E [nf, 3], (kx, ky) rad/um)."""
    dl = 0.02
    L_xy = 6 * dl
    pw = td.PlaneWave(center=(0, 0, -1.2), size=(td.inf, td.inf, 0), source_time=td.GaussianPulse(freq0=2e14, fwidth=4e13),
                      direction="+", angle_theta=THETA, angle_phi=PHI, pol_angle=0.0)
    structures = [] if medium is None else [
        td.Structure(geometry=td.Box(center=(0, 0, 0.005), size=(td.inf, td.inf, SLAB_D)), medium=medium)]
    sim = td.Simulation(
        size=(L_xy, L_xy, 4.0), grid_spec=td.GridSpec.uniform(dl=dl), run_time=6e-13, shutoff=0, subpixel=False,
        structures=structures, sources=[pw],
        monitors=[td.FluxMonitor(center=(0, 0, -1.6), size=(td.inf, td.inf, 0), freqs=list(FREQS), name="R"),
                  td.FluxMonitor(center=(0, 0, 1.2), size=(td.inf, td.inf, 0), freqs=list(FREQS), name="T"),
                  td.FieldMonitor(center=(0, 0, 1.2), size=(0, 0, 0), freqs=list(FREQS), name="pt", fields=["Ex", "Ey", "Ez"])],
        boundary_spec=td.BoundarySpec(x=td.Boundary.bloch_from_source(pw, L_xy, 0), y=td.Boundary.bloch_from_source(pw, L_xy, 1),
                                      z=td.Boundary.pml(num_layers=12)))
    disc = discretize(sim)
    with HipEngine(disc.spec, lib=lib) as e:
        e.run()
        sd = assemble(disc, e.results(), log="")
    probe = np.stack([getattr(sd["pt"], c).values.ravel() for c in ("Ex", "Ey", "Ez")], axis=1)
    kpar = np.array([disc.spec.bloch[0], disc.spec.bloch[1]]) / L_xy
    return sd["R"].flux.values.ravel(), sd["T"].flux.values.ravel(), probe, kpar


def slab_errors(lib, eps, medium, inc):
    """Worst deviation from the transfer matrix over FREQS: (co-polarised |t|, cross-polarised |t|, R, T, |R + T - 1|)."""
    fr, ft, probe, kpar = slab_run(lib, medium)
    t, r = berreman_slab(eps, SLAB_D, FREQS, kpar, "p")
    k0 = 2 * np.pi * FREQS / 2.99792458e14
    co, cross = [], []
    for i in range(len(FREQS)):
        (s_hat, p_hat), _ = vacuum_modes(kpar[0] / k0[i], kpar[1] / k0[i], 1)
        a_inc = np.linalg.norm(inc["probe"][i])
        co.append(abs(np.dot(p_hat, probe[i])) / a_inc)
        cross.append(abs(np.dot(s_hat, probe[i])) / a_inc)
    R, T = -fr / inc["T"], ft / inc["T"]
    return (np.abs(np.array(co) - np.abs(t[:, 1])).max(), np.abs(np.array(cross) - np.abs(t[:, 0])).max(),
            np.abs(R - np.sum(np.abs(r) ** 2, axis=1)).max(), np.abs(T - np.sum(np.abs(t) ** 2, axis=1)).max(),
            np.abs(R + T - 1).max())


def test_rotated_uniaxial_slab_under_oblique_light_matches_the_transfer_matrix(hip_lib):
    """The bar is the isotropic slab's own deviation, measured in the same run (on an MI355X: co |t| 9.8e-4, cross |t| 3e-5, R 4.0e-3,
    T 1.8e-3, |R + T - 1| 4.5e-3 — the flux planes' floor, lossless slab); the rotated uniaxial slab is held to twice it (at least
    1e-3 for the amplitudes, 2e-3 for R + T; measured 9.5e-4, 4.9e-5, 4.1e-3, 1.7e-3, 4.5e-3)."""
    _, ft, probe, kpar = slab_run(hip_lib, None)
    inc = {"T": ft, "probe": probe}
    k0 = 2 * np.pi * FREQS / 2.99792458e14
    for i in range(len(FREQS)):                            # the incident wave is p-polarised
        (s_hat, p_hat), _ = vacuum_modes(kpar[0] / k0[i], kpar[1] / k0[i], 1)
        assert abs(np.dot(s_hat, probe[i])) < 1e-3 * np.linalg.norm(probe[i])
    iso = slab_errors(hip_lib, N_ISO ** 2 * np.eye(3), td.Medium(permittivity=N_ISO ** 2), inc)
    eps = AXES @ np.diag([N_E ** 2, N_O ** 2, N_O ** 2]) @ AXES.T
    med = td.FullyAnisotropicMedium(permittivity=eps)
    ani = slab_errors(hip_lib, eps, med, inc)
    print("isotropic floor (co, cross, R, T, R+T-1):", ["%.2e" % v for v in iso])
    print("rotated uniaxial  (co, cross, R, T, R+T-1):", ["%.2e" % v for v in ani])
    assert max(iso) < 1e-2, iso
    for name, got, floor in zip(("co", "cross", "R", "T"), ani[:4], (iso[0], iso[0], iso[2], iso[3])):
        assert got < max(2 * floor, 1e-3), (name, got, floor)
    assert ani[4] < max(2 * iso[4], 2e-3), (ani[4], iso[4])
    t, _ = berreman_slab(eps, SLAB_D, FREQS, kpar, "p")
    assert np.abs(t[:, 0]).min() > 0.05                    # (a real polarisation conversion)



# ------------------------------------------------------------------------------------------------------------- (d) stability
def test_closed_lossless_bloch_cell_stays_bounded(hip_lib):
    disc = discretize(wrapped_cell(lossless=True, run_time=1e-11), n_steps=20400)
    assert any(np.abs(st.nbr_wrap).any() for st in disc.spec.aniso)
    with HipEngine(disc.spec, lib=hip_lib) as e:
        e.run(400)
        amp0 = max(float(np.abs(e.get_field(c)).max()) for c in range(3))
        st = e.run(20000)
        amp1 = max(float(np.abs(e.get_field(c)).max()) for c in range(3))
    assert int(st.diverged) == 0 and int(st.steps_done) == 20400
    assert np.isfinite(amp1) and 0 < amp1 < 3 * amp0, (amp0, amp1)
