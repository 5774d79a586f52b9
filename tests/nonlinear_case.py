"""Kerr media (Medium.nonlinear_spec, NonlinearSusceptibility): the fp64 reference and the scenarios shared by tests/test_emu_nonlinear.py
(emulator) and tests/test_gpu_nonlinear.py (device).  docs/history/NONLINEAR.md holds the scheme and the figures.

  reference  ``NonlinearOracle``: the fp64 oracle's own E update, then at the listed nodes num_iters Jacobi iterations of
                 E^(m) = alpha_m E^n + beta_m (E_lin - Ca E^n),   alpha_m = (eps_bar + chi3 I^n - s_bar) / (eps_bar + chi3 I^(m-1) + s_bar),
                                                                  beta_m  = (eps_bar + s_bar) / (eps_bar + chi3 I^(m-1) + s_bar)
             with eps_bar, s_bar from the oracle's own Ca / Cb arrays and the NonlinearSet of the spec.
  scenarios  five small grids, each started from the dense band-limited random state of tests/dense_state.py and run 1, 2 and 7 steps
             through the fused single steps and the two-pass kernels, num_iters 1 and 5.
  chi3       scaled per scenario from the state's own amplitude: max |chi3| I / eps_bar over the listed nodes is TARGET at the start
             and must lie in [0.05, 0.3] at the start and after every run the references take (``Scenario.strength``).
  bar        2e-5 rel-L2 per field against the fp64 reference (the bar of tests/test_gpu_parity.py).
  condition  the fp64 reference WITHOUT the lists differs from it by at least 100 x the bar on the listed nodes (``visibility``)."""
import dataclasses

import numpy as np

import tidy3d_amd.schema as td
from oracle.fdtd_numpy import OracleFdtd, _EPS0

import dense_state as ds
import list_case as lc
import modulation_case as mc
from cases import PULSE

BAR = 2e-5
KS = (1, 2, 7)
ITERS = (1, 5)
TARGET = 0.10             # max |chi3| I / eps_bar over the listed nodes of the initial state
RANGE = (0.05, 0.3)


def intensity(E, ns):
    """I at the nodes of ``ns`` from the three E arrays: E_a^2 + (mean of four E_b)^2 + (mean of four E_c)^2, a missing slot = 0"""
    i = (ns.ijk[:, 2], ns.ijk[:, 1], ns.ijk[:, 0])
    out = np.asarray(E[ns.comp][i], np.float64) ** 2
    for half in (0, 1):
        s = np.zeros(len(ns.ijk))
        for slot in range(4 * half, 4 * half + 4):
            j = ns.nbr_ijk[:, slot]
            ok = j[:, 0] >= 0
            s[ok] += E[ns.nbr_comp[slot]][j[ok, 2], j[ok, 1], j[ok, 0]]
        out = out + (0.25 * s) ** 2
    return out


class NonlinearOracle(OracleFdtd):
    """OracleFdtd with the Kerr fixed-point update at the nodes of ``spec.nonlinear``."""

    def update_e(self, n: int):
        sets = getattr(self.spec, "nonlinear", None) or []
        idx = [(s.ijk[:, 2], s.ijk[:, 1], s.ijk[:, 0]) for s in sets]
        e_old = [self.E[s.comp][i].copy() for s, i in zip(sets, idx)]
        i_old = [intensity(self.E, s) for s in sets]
        super().update_e(n)
        if not sets:
            return
        dt = self.spec.dt
        e_lin = [self.E[s.comp][i].copy() for s, i in zip(sets, idx)]
        coef = []
        for s, i in zip(sets, idx):
            c = s.comp
            ca = (self.ca[c][i] if np.ndim(self.ca[c]) else np.full(len(s.ijk), self.ca[c])).astype(np.float64)
            cb = (self.cb[c][i] if np.ndim(self.cb[c]) else np.full(len(s.ijk), self.cb[c])).astype(np.float64)
            eps_bar = dt / (_EPS0 * cb) * 2.0 / (1.0 + ca)
            coef.append((ca, eps_bar, eps_bar * (1.0 - ca) / (1.0 + ca)))
        for _ in range(int(sets[0].num_iters)):
            nxt = []
            for s, eo, io, el, (ca, eb, sb) in zip(sets, e_old, i_old, e_lin, coef):
                den = eb + s.chi3 * intensity(self.E, s) + sb
                alpha, beta = (eb + s.chi3 * io - sb) / den, (eb + sb) / den
                nxt.append(alpha * eo + beta * (el - ca * eo))
            for s, i, v in zip(sets, idx, nxt):          # Jacobi: all computed, then all stored
                self.E[s.comp][i] = v.astype(self.dtype)


# ---------------------------------------------------------------------------------------------------------------- media
def kerr(eps=4.0, chi3=1.0, num_iters=5, **kw):
    """chi3 here is RELATIVE: ``Scenario`` scales the lists of a spec by one factor found from its state"""
    return td.Medium(permittivity=eps, nonlinear_spec=td.NonlinearSpec(models=(td.NonlinearSusceptibility(chi3=chi3),), num_iters=num_iters), **kw)


def _bx(center, size, med):
    return td.Structure(geometry=td.Box(center=center, size=size), medium=med)


# (the dipole of tests/modulation_case.py at 2e-4 of its amplitude: what it injects in seven steps stays below the dense state — at
#  full amplitude it takes |chi3| I / eps_bar past 10^3 within seven steps and the fixed point out of its range)
WEAK = dataclasses.replace(PULSE, amplitude=2e-4 * PULSE.amplitude)
DIPOLE = dataclasses.replace(mc.DIPOLE, source_time=WEAK)


_PEC3 = lambda: td.BoundarySpec(x=mc._pec(), y=mc._pec(), z=mc._pec())      # noqa: E731


# ---------------------------------------------------------------------------------------------------------------- scenarios
def pec_box_blocks():
    """24 x 20 x 28 PEC box: a Kerr block (chi3 > 0) touching a plain dielectric and a Lorentz block, a block with chi3 < 0 touching the
    dielectric, a Kerr block with conductivity touching that one."""
    bodies = [_bx((-0.25, 0, 0.1), (0.3, 0.4, 0.5), kerr(eps=4.0, chi3=1.0)),
              _bx((0.25, 0, -0.1), (0.3, 0.4, 0.5), kerr(eps=2.5, chi3=-0.7)),
              _bx((0.25, -0.3, -0.1), (0.3, 0.2, 0.3), kerr(eps=3.0, chi3=0.5, conductivity=0.05)),
              _bx((0, 0, 0), (0.2, 0.3, 0.4), td.Medium(permittivity=3.0)),
              _bx((-0.25, 0.3, 0.1), (0.3, 0.2, 0.3), td.Lorentz(eps_inf=2.0, coeffs=[(1.5, 4e14, 3e13)]))]
    spec = mc._spec(mc._box_sim((24, 20, 28), _PEC3(), bodies, sources=(DIPOLE,)))
    assert spec.shape == (24, 20, 28)
    chi = np.concatenate([s.chi3 for s in spec.nonlinear])
    assert (chi < 0).any() and (chi > 0).any() and len(np.unique(chi)) == 3
    return spec


def seam_bar():
    """264 x 8 x 12: a Kerr bar from cell 244 across the x-tile seam at 256 into the partial tile."""
    from tidy3d_amd.discretize import discretize
    sim = mc._box_sim((264, 8, 12), _PEC3(), sources=(DIPOLE,))
    b = np.asarray(discretize(sim, n_steps=1).spec.boundaries[0])
    x0, x1 = float(b[244]), float(b[262])
    bar = _bx((0.5 * (x0 + x1), 0.02, 0.03), (x1 - x0, 0.2, 0.3), kerr(eps=3.0))
    spec = mc._spec(dataclasses.replace(sim, structures=[bar]))
    ii = np.concatenate([s.ijk[:, 0] for s in spec.nonlinear])
    assert spec.shape == (264, 8, 12) and ii.min() < ds.X_TILE - 2 and ii.max() >= ds.X_TILE + 2, (ii.min(), ii.max())
    return spec


def periodic_xy():
    """16 x 12 x 24, periodic in x and y, PEC z: the body runs through both periodic faces — neighbour slots wrap."""
    bspec = td.BoundarySpec(x=td.Boundary.periodic(), y=td.Boundary.periodic(), z=mc._pec())
    spec = mc._spec(mc._box_sim((16, 12, 24), bspec, [_bx((0, 0, 0.1), (td.inf, td.inf, 0.5), kerr(eps=3.0))], sources=(DIPOLE,)))
    assert spec.shape == (16, 12, 24)
    wrapped = 0
    for s in spec.nonlinear:
        assert (s.nbr_ijk >= 0).all() or s.comp != 2        # (only z walls leave a slot empty, and only E_x / E_y slots reach along z)
        d = s.nbr_ijk[:, :, :2] - s.ijk[:, None, :2]
        wrapped += int((np.abs(d) > 1).sum())
    assert wrapped > 0
    return spec


def pml_slab():
    """20 x 20 x 36: CPML on z (6 layers either side of 24 cells), periodic x and y; the Kerr slab reaches through the upper layers to
    the wall; a dipole inside the slab injects during the steps."""
    bspec = td.BoundarySpec(x=td.Boundary.periodic(), y=td.Boundary.periodic(), z=td.Boundary.pml(num_layers=6))
    slab = _bx((0, 0, 5.1), (td.inf, td.inf, 10.0), kerr(eps=2.5))
    src = [td.PointDipole(center=(0.03, -0.07, 0.3), source_time=WEAK, polarization="Ez")]
    spec = mc._spec(mc._box_sim((20, 20, 24), bspec, [slab], sources=src))
    assert spec.shape == (20, 20, 36)
    kk = np.concatenate([s.ijk[:, 2] for s in spec.nonlinear])
    assert kk.max() == 35 and len(spec.sources) == 1
    return spec


def graded_two_media():
    """A graded grid on all axes, sub-pixel averaging on; two Kerr media with different chi3 side by side: the nodes on the blocks' faces
    carry an averaged eps_bar."""
    dl_x = tuple(0.03 + 0.02 * np.abs(np.linspace(-1, 1, 20)))
    dl_y = tuple(0.04 + 0.015 * np.linspace(0, 1, 16))
    dl_z = tuple(0.05 - 0.015 * np.linspace(0, 1, 12))
    size = (float(np.sum(dl_x)), float(np.sum(dl_y)), float(np.sum(dl_z)))
    bodies = [_bx((-0.11, -0.02, 0.01), (0.23, 0.33, 0.26), kerr(eps=3.5, chi3=1.0)),
              _bx((0.125, -0.02, 0.01), (0.24, 0.33, 0.26), kerr(eps=2.2, chi3=-0.4))]
    sim = td.Simulation(size=size, grid_spec=td.GridSpec(grid_x=td.CustomGrid(dl=dl_x), grid_y=td.CustomGrid(dl=dl_y), grid_z=td.CustomGrid(dl=dl_z)),
                        run_time=1e-12, structures=bodies, sources=[DIPOLE], monitors=[], boundary_spec=_PEC3(), shutoff=0, subpixel=True)
    spec = mc._spec(sim)
    assert spec.shape == (20, 16, 12)
    chi = np.concatenate([s.chi3 for s in spec.nonlinear])
    eps_bar = np.concatenate([listed_eps(spec, s) for s in spec.nonlinear])
    assert len(np.unique(chi)) == 2 and ((np.abs(eps_bar - 3.5) > 1e-3) & (np.abs(eps_bar - 2.2) > 1e-3)).any()      # sub-pixel values among them
    return spec


def small_at_wall():
    """12 x 12 x 12 PEC box with a PMC wall at x- (8^3 leaves over 10 % of its nodes pinned: list_case.SHARE_CAP; across a PMC wall the
    nodes a slot beyond the x+ wall would wrap to are live, behind a PEC wall they are pinned and a wrongly filled slot reads 0), a Kerr body of 3 x 3 x 3 cells against the
    x+ wall: lists shorter than a wavefront, E_x nodes whose slots reach beyond the wall.  (Where the body lies decides whether the
    state keeps |chi3| I / eps_bar inside RANGE for seven steps; a body of 2 x 2 x 2 cells on the axis falls to 0.02.)"""
    body = _bx((4.5 * mc.DL, 0.5 * mc.DL, -0.5 * mc.DL), (3 * mc.DL,) * 3, kerr(eps=3.0))
    walls = td.BoundarySpec(x=td.Boundary(minus=td.PMCBoundary(), plus=td.PECBoundary()), y=mc._pec(), z=mc._pec())
    spec = mc._spec(mc._box_sim((12, 12, 12), walls, [body], sources=(DIPOLE,)))
    assert spec.shape == (12, 12, 12) and max(len(s.ijk) for s in spec.nonlinear) < 64
    return spec


SCENARIOS = {"pec_box_blocks": pec_box_blocks, "seam_bar": seam_bar, "periodic_xy": periodic_xy, "pml_slab": pml_slab,
             "graded_two_media": graded_two_media}
EXTRA = {"small_at_wall": small_at_wall}          # (not in the emulator's committed record)
PATHS = lc.PATHS
GOLDEN = lc.golden("nonlinear")


def listed_eps(spec, s):
    return np.asarray([spec.media[i].eps_inf for i in spec.mat_idx[s.comp][s.ijk[:, 2], s.ijk[:, 1], s.ijk[:, 0]]], np.float64)


def with_lists(spec, scale=1.0, num_iters=None, reverse=False):
    """the spec with chi3 of every list times ``scale``, another iteration count, or its lists in reversed node order"""
    out = []
    for s in spec.nonlinear:
        o = slice(None, None, -1) if reverse else slice(None)
        out.append(dataclasses.replace(s, ijk=np.ascontiguousarray(s.ijk[o]), nbr_ijk=np.ascontiguousarray(s.nbr_ijk[o]),
                                       chi3=np.ascontiguousarray(s.chi3[o] * scale), num_iters=int(num_iters or s.num_iters)))
    return dataclasses.replace(spec, nonlinear=out[::-1] if reverse else out)


class Scenario(lc.Scenario):
    """chi3 scaled to the state; the fp64 references per (K, num_iters)"""
    ATTR, TAG, ORACLE, SCENARIOS, BAR, GOLDEN = "nonlinear", "nonlinear", NonlinearOracle, SCENARIOS, BAR, GOLDEN
    EXTRA = EXTRA

    def __init__(self, label):
        super().__init__(label)
        s0 = self._strength(self.spec, self.state)
        assert s0 > 0
        self.spec = with_lists(self.spec, scale=TARGET / s0)

    @staticmethod
    def _strength(spec, fields):
        E = [np.asarray(f, np.float64) for f in fields[:3]]
        return max(float(np.max(np.abs(s.chi3) * intensity(E, s) / listed_eps(spec, s))) for s in spec.nonlinear)

    def strength(self, K=0):
        """max |chi3| I / eps_bar over the listed nodes, of the initial state (K = 0) or of the reference after K steps"""
        return self._strength(self.spec, self.state if K == 0 else self.ref(K))

    def ref_spec(self, num_iters):
        return with_lists(self.spec, num_iters=num_iters)

    def ref(self, K, num_iters=5):
        return super().ref(K, num_iters)

    def errors(self, fields, K, num_iters=5):
        return super().errors(fields, K, num_iters)

    def measure(self, fields, K, num_iters=5, ref=None):
        return super().measure(fields, K, num_iters, ref=ref)

    def floor(self, K, num_iters=5):
        return super().floor(K, num_iters)

    def bar_nodes(self, K, num_iters=5):
        return super().bar_nodes(K, num_iters)

    def check_nodes(self, fields, K, what, num_iters=5):
        return super().check_nodes(fields, K, what, num_iters)

    def run(self, lib, K, path, num_iters=5, plain=False, **kw):
        spec = self.plain if plain else with_lists(self.spec, num_iters=num_iters, **kw)
        return ds.run_engine(spec, lib, self.state, K, path)


def scenario(label):
    return lc.scenario(Scenario, label)


def emulator_record(lib):
    """(num_iters 5)"""
    return lc.emulator_record(Scenario, lib)


def check_against_emulator_record(label, fields):
    return lc.check_against_emulator_record(scenario(label), fields)


def check_scenario(lib, label, K, num_iters, what=""):
    """the chi3 condition; both paths under the bar; equal bits between them.  -> (worst error, fields per path)"""
    sc = scenario(label)
    for k in (0, K):
        s = sc.strength(k)
        assert RANGE[0] <= s <= RANGE[1], (label, k, s)
    got = {p: sc.run(lib, K, p, num_iters) for p in PATHS}
    worst = 0.0
    for p in PATHS:
        err = sc.errors(got[p].fields, K, num_iters)
        print(f"[nonlinear] {label} K={K} iters={num_iters} {what}{p}: rel-L2 per field " + " ".join(f"{e:.2e}" for e in err)
              + f" | off-reason {got[p].why}")
        worst = max(worst, max(err))
        sc.check_nodes(got[p].fields, K, what + p, num_iters)          # the same run, node by node: its message says where
        assert max(err) <= BAR, (label, K, num_iters, p, err)
    for c in range(6):
        assert np.array_equal(got["fused"].fields[c], got["twopass"].fields[c]), (label, K, num_iters, ds.COMP[c])
    return worst, got
