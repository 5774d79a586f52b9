"""Time-modulated media (Medium.modulation_spec): the fp64 reference and the scenarios shared by tests/test_emu_modulation.py (emulator)
and tests/test_gpu_modulation.py (device).  docs/history/MODULATION.md holds the scheme and the figures.

  reference  ``ModulatedOracle``: the fp64 oracle's own E update, then at the listed nodes
                 E^{n+1} = alpha E^n + beta (E_lin - Ca E^n),  alpha = (eps^n - s) / (eps^{n+1} + s),  beta = (eps_bar + s_bar) / (eps^{n+1} + s)
             with every coefficient derived from the oracle's own Ca / Cb arrays and the ModulationSet of the spec.
  scenarios  five small grids, each started from the dense band-limited random state of tests/dense_state.py and run 1, 2 and 7 steps
             (odd and even n, t != 0) through the fused single steps and the two-pass kernels.
  bar        2e-5 rel-L2 per field against the fp64 reference (the bar of tests/test_gpu_parity.py).
  condition  the fp64 reference WITHOUT the patch differs from it by at least 100 x the bar on the listed nodes (``visibility``): a
             scenario that cannot see the feature proves nothing."""
import dataclasses

import numpy as np

import tidy3d_amd.schema as td
from tidy3d_amd.data import DataArray
from tidy3d_amd.discretize import discretize
from oracle.fdtd_numpy import OracleFdtd, _EPS0

import dense_state as ds
import list_case as lc
from cases import DL, PULSE

BAR = 2e-5
KS = (1, 2, 7)
F_MOD = 1.0e15            # Hz: ~0.6 rad per time step at DL = 0.05 um — eps(t) moves by a sixth of its swing from one step to the next


class ModulatedOracle(OracleFdtd):
    """OracleFdtd with the time-modulated update at the nodes of ``spec.modulation``."""

    def update_e(self, n: int):
        spec = self.spec
        mods = getattr(spec, "modulation", None) or []
        idx = [(m.ijk[:, 2], m.ijk[:, 1], m.ijk[:, 0]) for m in mods]
        e_old = [self.E[m.comp][i].copy() for m, i in zip(mods, idx)]
        super().update_e(n)
        rd, dt = self.rdtype, spec.dt
        for m, i, eo in zip(mods, idx, e_old):
            c = m.comp
            ca = (self.ca[c][i] if np.ndim(self.ca[c]) else np.full(len(eo), self.ca[c])).astype(np.float64)
            cb = (self.cb[c][i] if np.ndim(self.cb[c]) else np.full(len(eo), self.cb[c])).astype(np.float64)
            eps_bar = dt / (_EPS0 * cb) * 2.0 / (1.0 + ca)
            s_bar = eps_bar * (1.0 - ca) / (1.0 + ca)
            we, ws = 2.0 * np.pi * m.freq_eps, 2.0 * np.pi * m.freq_sigma
            eps_n = eps_bar + np.real(m.d_eps * np.exp(-1j * we * n * dt))
            eps_n1 = eps_bar + np.real(m.d_eps * np.exp(-1j * we * (n + 1) * dt))
            s = s_bar + np.real(m.d_sigma * (dt / (2.0 * _EPS0)) * np.exp(-1j * ws * (n + 0.5) * dt))
            alpha = ((eps_n - s) / (eps_n1 + s)).astype(rd)
            beta = ((eps_bar + s_bar) / (eps_n1 + s)).astype(rd)
            e_lin = self.E[c][i]
            self.E[c][i] = (alpha * eo + beta * (e_lin - ca.astype(rd) * eo)).astype(self.dtype)


# ---------------------------------------------------------------------------------------------------------------- media
def cw(freq0=F_MOD, amplitude=1.0, phase=0.0):
    return td.ContinuousWaveTimeModulation(freq0=freq0, amplitude=amplitude, phase=phase)


def eps_modulated(eps=4.0, amp=1.0, freq0=F_MOD, phase=0.3, space=None, **kw):
    stm = td.SpaceTimeModulation(time_modulation=cw(freq0, amp, phase), space_modulation=space or td.SpaceModulation())
    return td.Medium(permittivity=eps, modulation_spec=td.ModulationSpec(permittivity=stm), **kw)


def sigma_modulated(eps=2.5, sigma=0.05, amp=0.04, freq0=0.7 * F_MOD, phase=-0.4):
    stm = td.SpaceTimeModulation(time_modulation=cw(freq0, amp, phase))
    return td.Medium(permittivity=eps, conductivity=sigma, modulation_spec=td.ModulationSpec(conductivity=stm))


def _pec():
    return td.Boundary(minus=td.PECBoundary(), plus=td.PECBoundary())


DIPOLE = td.PointDipole(center=(0.03, -0.07, 0.01), source_time=PULSE, polarization="Ez")


def _box_sim(N, bspec, structures=(), sources=(DIPOLE,)):
    """exactly N cells of DL per axis (CPML layers are added to them), centred on the origin"""
    grid = td.GridSpec(grid_x=td.CustomGrid(dl=(DL,) * N[0]), grid_y=td.CustomGrid(dl=(DL,) * N[1]), grid_z=td.CustomGrid(dl=(DL,) * N[2]))
    return td.Simulation(size=tuple(float(np.sum((DL,) * n)) for n in N), grid_spec=grid, run_time=1e-12, structures=list(structures),
                         sources=list(sources), monitors=[], boundary_spec=bspec, shutoff=0)


def _spec(sim, n_steps=max(KS)):
    spec = discretize(sim, n_steps=n_steps).spec
    spec.decay_every = 0
    return spec


# ---------------------------------------------------------------------------------------------------------------- scenarios
def pec_box_blocks():
    """24 x 20 x 28 PEC box: a permittivity-modulated block (uniform amplitude) and a conductivity-modulated block with sigma_bar > 0,
    both strictly inside, a plain dielectric touching both."""
    bodies = [td.Structure(geometry=td.Box(center=(-0.25, 0, 0.1), size=(0.3, 0.4, 0.5)), medium=eps_modulated()),
              td.Structure(geometry=td.Box(center=(0.25, 0, -0.1), size=(0.3, 0.4, 0.5)), medium=sigma_modulated()),
              td.Structure(geometry=td.Box(center=(0, 0, 0), size=(0.2, 0.3, 0.4)), medium=td.Medium(permittivity=3.0))]
    spec = _spec(_box_sim((24, 20, 28), td.BoundarySpec(x=_pec(), y=_pec(), z=_pec()), bodies))
    assert spec.shape == (24, 20, 28)
    return spec


def seam_bar():
    """264 x 8 x 12: a modulated bar from cell 244 across the x-tile seam at 256 into the partial tile."""
    sim = _box_sim((264, 8, 12), td.BoundarySpec(x=_pec(), y=_pec(), z=_pec()))
    b = np.asarray(discretize(sim, n_steps=1).spec.boundaries[0])
    x0, x1 = float(b[244]), float(b[262])
    bar = td.Structure(geometry=td.Box(center=(0.5 * (x0 + x1), 0.02, 0.03), size=(x1 - x0, 0.2, 0.3)), medium=eps_modulated(eps=3.0, amp=0.8))
    spec = _spec(dataclasses.replace(sim, structures=[bar]))
    ii = np.concatenate([m.ijk[:, 0] for m in spec.modulation])
    assert spec.shape == (264, 8, 12) and ii.min() < ds.X_TILE - 2 and ii.max() >= ds.X_TILE + 2, (ii.min(), ii.max())
    return spec


def pml_slab():
    """20 x 20 x 36: CPML on z (6 layers either side of 24 cells), periodic x and y; the modulated slab reaches through the upper
    layers to the wall; a dipole inside the slab injects during the steps."""
    bspec = td.BoundarySpec(x=td.Boundary.periodic(), y=td.Boundary.periodic(), z=td.Boundary.pml(num_layers=6))
    slab = td.Structure(geometry=td.Box(center=(0, 0, 5.1), size=(td.inf, td.inf, 10.0)), medium=eps_modulated(eps=2.5, amp=0.6))
    src = [td.PointDipole(center=(0.03, -0.07, 0.3), source_time=PULSE, polarization="Ez")]
    spec = _spec(_box_sim((20, 20, 24), bspec, [slab], sources=src))
    assert spec.shape == (20, 20, 36)
    kk = np.concatenate([m.ijk[:, 2] for m in spec.modulation])
    assert kk.max() == 35 and len(spec.sources) == 1                  # through the layers to the wall
    return spec


def graded_travelling_wave():
    """A graded grid on all axes; the modulation's amplitude and phase are SpatialDataArrays — a phase ramp along x: a travelling-wave
    modulation — interpolated linearly at every component's own Yee nodes; sub-pixel averaging on: the nodes on the block's faces
    carry an averaged eps_bar."""
    dl_x = tuple(0.03 + 0.02 * np.abs(np.linspace(-1, 1, 20)))
    dl_y = tuple(0.04 + 0.015 * np.linspace(0, 1, 16))
    dl_z = tuple(0.05 - 0.015 * np.linspace(0, 1, 12))
    size = (float(np.sum(dl_x)), float(np.sum(dl_y)), float(np.sum(dl_z)))
    xs, ys, zs = np.linspace(-0.3, 0.3, 7), np.linspace(-0.2, 0.2, 3), np.linspace(-0.15, 0.15, 3)
    amp = 0.6 + 0.4 * np.cos(3.0 * xs)[:, None, None] * np.ones((1, 3, 1)) * (1.0 + 0.2 * zs / 0.15)[None, None, :]
    phase = (2.0 * np.pi * xs / 0.45)[:, None, None] * np.ones((1, 3, 3))
    coords = {"x": xs, "y": ys, "z": zs}
    space = td.SpaceModulation(amplitude=DataArray(amp, coords), phase=DataArray(phase, coords), interp_method="linear")
    assert float(amp.max()) <= 1.2
    body = td.Structure(geometry=td.Box(center=(0.01, -0.02, 0.01), size=(0.47, 0.33, 0.26)), medium=eps_modulated(eps=3.5, amp=1.0, space=space))
    sim = td.Simulation(size=size, grid_spec=td.GridSpec(grid_x=td.CustomGrid(dl=dl_x), grid_y=td.CustomGrid(dl=dl_y), grid_z=td.CustomGrid(dl=dl_z)),
                        run_time=1e-12, structures=[body], sources=[DIPOLE],
                        monitors=[], boundary_spec=td.BoundarySpec(x=_pec(), y=_pec(), z=_pec()), shutoff=0, subpixel=True)
    spec = _spec(sim)
    assert spec.shape == (20, 16, 12)
    d = np.concatenate([m.d_eps for m in spec.modulation])
    assert np.ptp(np.abs(d)) > 0.1 and np.ptp(np.angle(d)) > 1.0      # amplitude and phase do vary over the nodes
    eps_bar = np.concatenate([np.asarray([spec.media[i].eps_inf for i in spec.mat_idx[m.comp][m.ijk[:, 2], m.ijk[:, 1], m.ijk[:, 0]]])
                              for m in spec.modulation])
    assert (np.abs(eps_bar - 3.5) > 1e-3).any()                       # sub-pixel values among the listed nodes
    return spec


def bloch_xy():
    """16 x 12 x 24: Bloch x (phase 0.7), periodic y, PEC z, through fdtd_run_bloch: the same lists on both handles."""
    bspec = td.BoundarySpec(x=td.Boundary(minus=td.BlochBoundary(bloch_vec=0.7 / (2 * np.pi)), plus=td.BlochBoundary(bloch_vec=0.7 / (2 * np.pi))),
                            y=td.Boundary.periodic(), z=_pec())
    # (the body crosses the Bloch faces: its nodes next to the ghost cells are listed)
    body = td.Structure(geometry=td.Box(center=(0, 0, 0.1), size=(td.inf, 0.3, 0.5)), medium=eps_modulated(eps=3.0, amp=0.9))
    spec = _spec(_box_sim((16, 12, 24), bspec, [body]))
    assert spec.shape == (16, 12, 24)
    assert spec.bloch is not None and abs(spec.bloch[0] - 0.7) < 1e-12 and spec.bloch[1] == 0.0
    return spec


def small_at_wall():
    """12 x 12 x 12 PEC box with a PMC wall at x- (8^3 leaves over 10 % of its nodes pinned: list_case.SHARE_CAP), a modulated body of 2 x 2 x 2 cells
    against the x+ wall: lists shorter than a wavefront"""
    body = td.Structure(geometry=td.Box(center=(5 * DL, 0.0, 0.0), size=(2 * DL,) * 3), medium=eps_modulated(eps=3.0, amp=0.8))
    walls = td.BoundarySpec(x=td.Boundary(minus=td.PMCBoundary(), plus=td.PECBoundary()), y=_pec(), z=_pec())
    spec = _spec(_box_sim((12, 12, 12), walls, [body]))
    assert spec.shape == (12, 12, 12) and max(len(m.ijk) for m in spec.modulation) < 64
    return spec


SCENARIOS = {"pec_box_blocks": pec_box_blocks, "seam_bar": seam_bar, "pml_slab": pml_slab, "graded_travelling_wave": graded_travelling_wave,
             "bloch_xy": bloch_xy}
EXTRA = {"small_at_wall": small_at_wall}          # (not in the emulator's committed record)
PATHS = lc.PATHS
GOLDEN = lc.golden("modulation")


class Scenario(lc.Scenario):
    ATTR, TAG, ORACLE, SCENARIOS, BAR, GOLDEN = "modulation", "modulation", ModulatedOracle, SCENARIOS, BAR, GOLDEN
    EXTRA = EXTRA


def scenario(label):
    return lc.scenario(Scenario, label)


def emulator_record(lib):
    return lc.emulator_record(Scenario, lib)


def check_against_emulator_record(label, fields):
    return lc.check_against_emulator_record(scenario(label), fields)


def check_scenario(lib, label, K, what=""):
    """both paths under the bar; the modulated runs equal bit for bit wherever the plain runs of the same spec are.
    -> (worst error, fields per path)"""
    sc = scenario(label)
    got = {p: sc.run(lib, K, p) for p in PATHS}
    worst = 0.0
    for p in PATHS:
        err = sc.errors(got[p].fields, K)
        print(f"[modulation] {label} K={K} {what}{p}: rel-L2 per field " + " ".join(f"{e:.2e}" for e in err) + f" | off-reason {got[p].why}")
        worst = max(worst, max(err))
        sc.check_nodes(got[p].fields, K, what + p)          # the same run, node by node: its message says where
        assert max(err) <= BAR, (label, K, p, err)
    lin = {p: sc.run(lib, K, p, plain=True) for p in PATHS}
    if all(np.array_equal(lin["fused"].fields[c], lin["twopass"].fields[c]) for c in range(6)):
        for c in range(6):
            assert np.array_equal(got["fused"].fields[c], got["twopass"].fields[c]), (label, K, ds.COMP[c])
    else:
        assert label != "bloch_xy"      # (Bloch x, periodic y, PEC z: tests/test_emu_fused.py holds the linear sweeps to equal bits)
        print(f"[modulation] {label} K={K}: the plain sweeps of this spec differ between the paths; no bit comparison")
    return worst, got
