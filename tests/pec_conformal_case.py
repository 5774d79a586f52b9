"""PEC-conformal boundaries (SubpixelSpec.pec = PECConformal): the fp64 reference, the operator matrices and the scenarios shared by
tests/test_emu_pec_conformal.py (CPU, emulator) and tests/test_gpu_pec_conformal.py (device).  docs/history/PEC_CONFORMAL.md holds
the scheme and the figures.

  reference  ``ConformalOracle``: the fp64 oracle's own H update, then at the listed faces
                 H_c += -(dt / mu0) sum_k s_k (l_k / A_eff - 1) / step_k E_k^n
             with the weights formed in double from ``l``, ``area_eff`` and the grid's boundaries — not from the float32 ``d``.
  operators  ``update_matrices``: W_h (conformal weights included) and W_e as scipy sparse matrices of lossless specs with PEC or
             periodic faces; E^{n+1} - 2 E^n + E^{n-1} = -W_e W_h E^n, so the leapfrog limit is: every eigenvalue of W_e W_h below 4.
  scenarios  small grids, each started from the dense random state of tests/dense_state.py and run 1, 2 and 7 steps through the
             fused single steps and the two-pass kernels; bar 2e-5 rel-L2 per field.
  condition  the fp64 oracle WITHOUT the correction differs from the reference by at least 2e-3 over the listed H nodes after one
             step (``visibility``)."""
import dataclasses

import numpy as np

import tidy3d_amd.schema as td
from tidy3d_amd.discretize import discretize
from oracle.fdtd_numpy import OracleFdtd, _EPS0, _MU0, _C0

import dense_state as ds
import list_case as lc
from cases import DL, PULSE

BAR = 2e-5
VISIBLE = 2e-3
KS = (1, 2, 7)
CONFORMAL = td.SubpixelSpec(pec=td.PECConformal())
STAIRCASE = td.SubpixelSpec(pec=td.Staircasing())
SIGN = (1.0, -1.0, -1.0, 1.0)


def double_weights(spec, cs):
    """[n, 4] float64: what H of the faces of ``cs`` gains per unit E of the four edges — from l, area_eff and the boundaries"""
    c = cs.comp - 3
    a1, a2 = (c + 1) % 3, (c + 2) % 3
    step = [np.diff(np.asarray(spec.boundaries[a], np.float64)) for a in range(3)]
    inv = np.stack([1.0 / step[a1][cs.ijk[:, a1]]] * 2 + [1.0 / step[a2][cs.ijk[:, a2]]] * 2, axis=1)
    w = -(spec.dt / _MU0) * np.asarray(SIGN)[None, :] * (cs.l / cs.area_eff[:, None] - 1.0) * inv
    w[cs.nbr_ijk[:, :, 0] < 0] = 0.0
    return w


class ConformalOracle(OracleFdtd):
    """OracleFdtd with the conformal H update at the faces of ``spec.conformal``."""

    def update_h(self, n: int):
        add = []
        for cs in getattr(self.spec, "conformal", None) or []:
            w = double_weights(self.spec, cs)
            d = np.zeros(len(cs.ijk), self.dtype)
            for k in range(4):
                j = cs.nbr_ijk[:, k]
                ok = j[:, 0] >= 0
                d[ok] += (w[ok, k] * self.E[cs.nbr_comp[k]][j[ok, 2], j[ok, 1], j[ok, 0]]).astype(self.dtype)
            add.append(d)
        super().update_h(n)
        for cs, d in zip(self.spec.conformal, add):
            self.H[cs.comp - 3][cs.ijk[:, 2], cs.ijk[:, 1], cs.ijk[:, 0]] += d


# ---------------------------------------------------------------------------------------------------------------- operators
def update_matrices(spec):
    """-> (W_h, W_e): H^{n+1/2} = H^{n-1/2} - W_h E^n, E^{n+1} = E^n + W_e H^{n+1/2} of a lossless spec without layers, fields
    stacked (x, y, z components, each [z, y, x] flattened)."""
    import scipy.sparse as sp
    from tidy3d_amd.spec import BC_PEC, BC_PERIODIC
    nx, ny, nz = spec.shape
    N = (nx, ny, nz)
    n = nx * ny * nz
    o = OracleFdtd(spec)
    assert not any(o.has_pml) and spec.absorber is None and not o.ade and spec.bloch is None

    def d1(a, fwd):
        per = spec.bc[a][0] == BC_PERIODIC
        m = sp.lil_matrix((N[a], N[a]))
        inv = (o.ip if fwd else o.id)[a].reshape(-1)
        for i in range(N[a]):
            j = i + 1 if fwd else i - 1
            m[i, i] = -inv[i] if fwd else inv[i]
            if 0 <= j < N[a] or per:
                m[i, j % N[a]] += inv[i] if fwd else -inv[i]
        return m.tocsr()

    def full(a, fwd):
        mats = [sp.identity(N[2]), sp.identity(N[1]), sp.identity(N[0])]
        mats[2 - a] = d1(a, fwd)
        return sp.kron(mats[0], sp.kron(mats[1], mats[2])).tocsr()

    zero = sp.csr_matrix((n, n))
    rows_h, rows_e = [], []
    for c in range(3):
        a1, a2 = (c + 1) % 3, (c + 2) % 3
        blk = [zero, zero, zero]
        blk[a2] = full(a1, True)
        blk[a1] = -full(a2, True)
        rows_h.append(sp.hstack(blk))
        blk = [zero, zero, zero]
        blk[a2] = full(a1, False)
        blk[a1] = -full(a2, False)
        cb = np.broadcast_to(np.asarray(o.cb[c], np.float64), (nz, ny, nx)).copy()
        for a in range(3):                                 # E tangential to a PEC min wall is pinned
            if a != c and spec.bc[a][0] == BC_PEC:
                sl = [slice(None)] * 3
                sl[2 - a] = 0
                cb[tuple(sl)] = 0.0
        rows_e.append(sp.diags(cb.reshape(-1)) @ sp.hstack(blk))
    live = sp.diags(np.concatenate([(np.broadcast_to(np.asarray(o.cb[c]), (nz, ny, nx)) != 0).reshape(-1) for c in range(3)]).astype(float))
    W_h = float(o.ch) * sp.vstack(rows_h).tocsr() @ live
    r, q, v = [], [], []
    for cs in getattr(spec, "conformal", None) or []:
        w = double_weights(spec, cs)
        f = (cs.comp - 3) * n + (cs.ijk[:, 2] * ny + cs.ijk[:, 1]) * nx + cs.ijk[:, 0]
        for k in range(4):
            j = cs.nbr_ijk[:, k]
            ok = j[:, 0] >= 0
            r.append(f[ok])
            q.append(cs.nbr_comp[k] * n + (j[ok, 2] * ny + j[ok, 1]) * nx + j[ok, 0])
            v.append(-w[ok, k])                            # (H -= W_h E)
    if r:
        W_h = W_h + sp.csr_matrix((np.concatenate(v), (np.concatenate(r), np.concatenate(q))), shape=(3 * n, 3 * n)) @ live
    return W_h.tocsr(), sp.vstack(rows_e).tocsr()


def largest_eigenvalue(spec):
    from scipy.sparse.linalg import eigs
    W_h, W_e = update_matrices(spec)
    rng = np.random.default_rng(3)
    lam = eigs((W_e @ W_h).tocsc(), k=1, which="LM", v0=rng.normal(size=W_h.shape[0]), tol=1e-9, maxiter=20000, return_eigenvectors=False)
    return float(np.abs(lam[0]))


def _pec():
    return td.Boundary(minus=td.PECBoundary(), plus=td.PECBoundary())


def _box_sim(N, bspec, structures=(), sources=(), subpixel=CONFORMAL, dl=DL):
    """exactly N cells of dl per axis (CPML layers are added to them), centred on the origin"""
    grid = td.GridSpec(grid_x=td.CustomGrid(dl=(dl,) * N[0]), grid_y=td.CustomGrid(dl=(dl,) * N[1]), grid_z=td.CustomGrid(dl=(dl,) * N[2]))
    return td.Simulation(size=tuple(float(np.sum((dl,) * n)) for n in N), grid_spec=grid, run_time=1e-12, structures=list(structures),
                         sources=list(sources), monitors=[], boundary_spec=bspec, shutoff=0, subpixel=subpixel)


def _spec(sim, n_steps=max(KS), clamp=None):
    if clamp is None:
        spec = discretize(sim, n_steps=n_steps).spec
    else:                                                  # the clamp's counter-example: the same pass with another factor
        import tidy3d_amd.conformal as cf
        keep = cf.CLAMP_FACTOR
        try:
            cf.CLAMP_FACTOR = clamp
            spec = discretize(sim, n_steps=n_steps).spec
        finally:
            cf.CLAMP_FACTOR = keep
    spec.decay_every = 0
    return spec


PEC_WALLS = td.BoundarySpec(x=_pec(), y=_pec(), z=_pec())


def sphere_in_box(offset, clamp=None, subpixel=CONFORMAL):
    """a PEC sphere of radius 5.3 cells in a 16^3 PEC box, its centre ``offset`` (cells) off the box's"""
    body = td.Structure(geometry=td.Sphere(center=tuple(float(v) * DL for v in offset), radius=5.3 * DL), medium=td.PEC)
    return _spec(_box_sim((16, 16, 16), PEC_WALLS, [body], subpixel=subpixel), clamp=clamp)


def cylinder_in_box(axis, offset, clamp=None):
    """a PEC cylinder of radius 4.3 cells along ``axis`` through a 14^3 PEC box"""
    body = td.Structure(geometry=td.Cylinder(center=tuple(float(v) * DL for v in offset), radius=4.3 * DL, length=td.inf, axis=axis), medium=td.PEC)
    return _spec(_box_sim((14, 14, 14), PEC_WALLS, [body]), clamp=clamp)


KA_TM010, KA_TE11 = 2.404825557695773, 1.841183781340659


def cavity_errors(a_cells, offset, subpixel):
    """relative errors of the TM010 and TE11 resonances of a circular vacuum cavity of radius ``a_cells`` cells: a PEC box with a
    vacuum cylinder on top of it as a later structure, the axis along a periodic z of one cell"""
    from scipy.sparse.linalg import eigs
    n = 2 * (a_cells + 2)
    size = n * DL
    bodies = [td.Structure(geometry=td.Box(center=(0, 0, 0), size=(2 * size, 2 * size, td.inf)), medium=td.PEC),
              td.Structure(geometry=td.Cylinder(center=(offset[0] * DL, offset[1] * DL, 0.0), radius=a_cells * DL, length=td.inf, axis=2),
                           medium=td.Medium(permittivity=1.0))]
    bspec = td.BoundarySpec(x=_pec(), y=_pec(), z=td.Boundary.periodic())
    spec = _spec(_box_sim((n, n, 1), bspec, bodies, subpixel=subpixel))
    assert bool(spec.conformal) == (subpixel is CONFORMAL)
    W_h, W_e = update_matrices(spec)
    M = (W_e @ W_h).tocsc()
    out = []
    for ka in (KA_TM010, KA_TE11):
        w = _C0 * ka / (a_cells * DL)
        target = (2.0 / spec.dt * np.sin(0.5 * w * spec.dt)) ** 2 * spec.dt ** 2          # the eigenvalue of W_e W_h an exact mode would have
        lam = eigs(M, k=4, sigma=target, which="LM", return_eigenvectors=False, tol=1e-10)
        lam = lam[np.argmin(np.abs(lam - target))]
        got = 2.0 / spec.dt * np.arcsin(0.5 * np.sqrt(float(np.real(lam))))
        out.append(abs(got - w) / w)
    return out


# ---------------------------------------------------------------------------------------------------------------- scenarios
def sphere_blocks():
    """24 x 20 x 28, PEC walls: an off-centre PEC sphere of radius 6.3 cells, a dielectric block and a Lorentz block touching it"""
    bodies = [td.Structure(geometry=td.Box(center=(-0.35, 0.05, 0.1), size=(0.3, 0.4, 0.5)), medium=td.Medium(permittivity=3.0)),
              td.Structure(geometry=td.Box(center=(0.3, -0.1, -0.2), size=(0.3, 0.4, 0.5)), medium=td.Lorentz(eps_inf=2.0, coeffs=[(1.5, 4e14, 3e13)])),
              td.Structure(geometry=td.Sphere(center=(0.043, -0.031, 0.067), radius=6.3 * DL), medium=td.PEC)]
    spec = _spec(_box_sim((24, 20, 28), PEC_WALLS, bodies))
    assert spec.shape == (24, 20, 28) and len(spec.media) >= 4
    return spec


def seam_cylinder():
    """264 x 12 x 12: a PEC cylinder of radius 3.4 cells along x across the seam between the 256-cell x tiles"""
    sim = _box_sim((264, 12, 12), PEC_WALLS)
    b = np.asarray(discretize(sim, n_steps=1).spec.boundaries[0])
    x0, x1 = float(b[244]) + 0.3 * DL, float(b[262]) - 0.4 * DL
    body = td.Structure(geometry=td.Cylinder(center=(0.5 * (x0 + x1), 0.013, -0.021), radius=3.4 * DL, length=x1 - x0, axis=0), medium=td.PEC)
    spec = _spec(dataclasses.replace(sim, structures=[body]))
    ii = np.concatenate([c.ijk[:, 0] for c in spec.conformal])
    assert spec.shape == (264, 12, 12) and ii.min() < ds.X_TILE - 2 and ii.max() >= ds.X_TILE + 2, (ii.min(), ii.max())
    return spec


def pml_tilted_slab():
    """20 x 20 x 36: periodic x and y, CPML in z (6 layers either side of 24 cells), a tilted PEC slab through the upper z layers to
    the wall, a live dipole.  Listed faces appear only outside the layers."""
    bspec = td.BoundarySpec(x=td.Boundary.periodic(), y=td.Boundary.periodic(), z=td.Boundary.pml(num_layers=6))
    zs = 18 * DL
    verts = [(-0.22, 0.1), (0.16, 0.1 + 0.38 * 0.35), (0.16 + 0.12, 0.1 + 0.38 * 0.35 - 0.12 / 0.35 * 0.1), (-0.22 + 0.12, 0.1 - 0.12 / 0.35 * 0.1)]
    slab = td.Structure(geometry=td.PolySlab(vertices=verts, axis=2, slab_bounds=(-0.21, zs + 1.0)), medium=td.PEC)
    src = [td.PointDipole(center=(0.03, -0.27, -0.3), source_time=PULSE, polarization="Ez")]
    spec = _spec(_box_sim((20, 20, 24), bspec, [slab], sources=src))
    assert spec.shape == (20, 20, 36) and len(spec.sources) == 1
    kk = np.concatenate([c.ijk[:, 2] for c in spec.conformal])
    assert kk.min() >= 6 and kk.max() <= 29 and (spec.mat_idx[:, 35] == 0).any()       # outside the layers; the slab reaches the wall
    return spec


def graded_sphere():
    """20 x 16 x 12, a graded grid on every axis: a PEC sphere, sub-pixel averaging of a dielectric sphere beside it"""
    dl_x = tuple(0.03 + 0.02 * np.abs(np.linspace(-1, 1, 20)))
    dl_y = tuple(0.04 + 0.015 * np.linspace(0, 1, 16))
    dl_z = tuple(0.05 - 0.015 * np.linspace(0, 1, 12))
    size = (float(np.sum(dl_x)), float(np.sum(dl_y)), float(np.sum(dl_z)))
    bodies = [td.Structure(geometry=td.Sphere(center=(0.17, 0.05, 0.01), radius=0.15), medium=td.Medium(permittivity=3.5)),
              td.Structure(geometry=td.Sphere(center=(-0.13, -0.04, 0.02), radius=0.17), medium=td.PEC)]
    sim = td.Simulation(size=size, grid_spec=td.GridSpec(grid_x=td.CustomGrid(dl=dl_x), grid_y=td.CustomGrid(dl=dl_y), grid_z=td.CustomGrid(dl=dl_z)),
                        run_time=1e-12, structures=bodies, sources=[], monitors=[], boundary_spec=PEC_WALLS, shutoff=0, subpixel=CONFORMAL)
    spec = _spec(sim)
    assert spec.shape == (20, 16, 12) and any(m.name.startswith("subpixel_") for m in spec.media)
    return spec


def periodic_sphere():
    """16^3, periodic on all axes: a PEC sphere (and its periodic image) across the x and z faces: listed faces with wrapped edges"""
    per = td.Boundary.periodic()
    c0 = (7.6 * DL, 0.02, 7.8 * DL)
    bodies = [td.Structure(geometry=td.Sphere(center=(c0[0] - sx * 16 * DL, c0[1], c0[2] - sz * 16 * DL), radius=4.3 * DL), medium=td.PEC)
              for sx in (0, 1) for sz in (0, 1)]
    spec = _spec(_box_sim((16, 16, 16), td.BoundarySpec(x=per, y=per, z=per), bodies))
    wrapped = sum(int(((cs.nbr_ijk[:, :, a] >= 0) & (cs.nbr_ijk[:, :, a] < cs.ijk[:, None, a])).sum()) for cs in spec.conformal for a in range(3))
    assert spec.shape == (16, 16, 16) and wrapped > 0
    return spec


def small_at_wall():
    """12 x 12 x 12 PEC box with a PMC wall at x- (8^3 leaves over 10 % of its nodes pinned: list_case.SHARE_CAP; across a PMC wall the
    edges a slot beyond the x+ wall would wrap to are live), a PEC sphere of radius 1.4 cells through the
    x+ wall: lists shorter than a wavefront, faces whose edges lie beyond the wall"""
    body = td.Structure(geometry=td.Sphere(center=(4.9 * DL, 0.1 * DL, -0.2 * DL), radius=1.4 * DL), medium=td.PEC)
    walls = td.BoundarySpec(x=td.Boundary(minus=td.PMCBoundary(), plus=td.PECBoundary()), y=_pec(), z=_pec())
    spec = _spec(_box_sim((12, 12, 12), walls, [body]))
    assert spec.shape == (12, 12, 12) and max(len(c.ijk) for c in spec.conformal) < 64
    return spec


SCENARIOS = {"sphere_blocks": sphere_blocks, "seam_cylinder": seam_cylinder, "pml_tilted_slab": pml_tilted_slab,
             "graded_sphere": graded_sphere, "periodic_sphere": periodic_sphere}
EXTRA = {"small_at_wall": small_at_wall}          # (not in the emulator's committed record)
# label -> (scenario, axis_shift): the first scenario under the other two axis renamings as well
RUNS = {**{k: (k, 0) for k in (*SCENARIOS, *EXTRA)}, "sphere_blocks_shift1": ("sphere_blocks", 1), "sphere_blocks_shift2": ("sphere_blocks", 2)}
PATHS = lc.PATHS
GOLDEN = lc.golden("pec_conformal")


class Scenario(lc.Scenario):
    ATTR, TAG, ORACLE, SCENARIOS, BAR, GOLDEN = "conformal", "pec-conformal", ConformalOracle, SCENARIOS, BAR, GOLDEN
    EXTRA = EXTRA


def scenario(label):
    return lc.scenario(Scenario, label)


def emulator_record(lib):
    return lc.emulator_record(Scenario, lib)


def check_against_emulator_record(label, fields):
    return lc.check_against_emulator_record(scenario(label), fields)


def check_run(lib, run_label, K, what=""):
    """both paths under the bar; the conformal runs equal bit for bit wherever the plain sweeps of the same spec are.
    -> (worst error, fields per path)"""
    label, shift = RUNS[run_label]
    sc = scenario(label)
    got = {p: sc.run(lib, K, p, axis_shift=shift) for p in PATHS}
    worst = 0.0
    for p in PATHS:
        err = sc.errors(got[p].fields, K)
        print(f"[pec-conformal] {run_label} K={K} {what}{p}: rel-L2 per field " + " ".join(f"{e:.2e}" for e in err) + f" | off-reason {got[p].why}")
        worst = max(worst, max(err))
        sc.check_nodes(got[p].fields, K, what + p + (f" shift {shift}" if shift else ""))          # the same run, node by node: its message says where
        assert max(err) <= BAR, (run_label, K, p, err)
    lin = {p: sc.run(lib, K, p, plain=True, axis_shift=shift) for p in PATHS}
    if all(np.array_equal(lin["fused"].fields[c], lin["twopass"].fields[c]) for c in range(6)):
        for c in range(6):
            assert np.array_equal(got["fused"].fields[c], got["twopass"].fields[c]), (run_label, K, ds.COMP[c])
    else:
        print(f"[pec-conformal] {run_label} K={K}: the plain sweeps of this spec differ between the paths; no bit comparison")
    return worst, got
