"""The off-diagonal coupling lists of FullyAnisotropicMedium (spec.AnisoSet, csrc/fdtd_aniso.hpp) held to the fp64 oracle node by node
where their slots reach across a periodic or Bloch face: the scenarios shared by tests/test_aniso_nodes.py (reference side, CPU),
tests/test_emu_aniso_nodes.py (emulator) and tests/test_gpu_aniso_nodes.py (device).  docs/history/ANISO_WRAPS.md holds the figures.

  reference  ``OracleFdtd`` itself: its anisotropic block rotates the curl recovered through a slot that crossed Bloch faces by
             exp(+i sum_a s_a phi_a), s = nbr_wrap.  That factor is pinned without any engine by ``oracle_translation``: the corner cell
             against the same cell with its window moved by half a period, where no slot crosses and the factor is never formed.
  scenarios  six small cells, each started from the dense state of tests/dense_state.py (complex under Bloch phases, seed 1) and run
             1, 2 and 7 steps through the fused single steps and the two-pass kernels; no run may take a step pair.
  measure    ``list_case.Scenario.check_nodes``: every node under ds.MARGIN x the floor of the fp32 oracle of the same scenario and K."""
import dataclasses

import numpy as np

import tidy3d_amd.schema as td
from tidy3d_amd.discretize import discretize
from oracle.fdtd_numpy import OracleFdtd

import dense_state as ds
import list_case as lc
import modulation_case as mc
import test_aniso_bloch as tab

KS = (1, 2, 7)
PATHS = lc.PATHS
DL = tab.DL
AX = "xyz"
BLOCH3 = (0.23, -0.31, 0.17)          # Bloch vectors (units of 2 pi / period): phases 1.445, -1.948, 1.068 rad


def _spec(sim, n_steps=max(KS)):
    spec = discretize(sim, n_steps=n_steps).spec
    spec.decay_every = 0
    return spec


def _faces(kinds, bloch=BLOCH3):
    """per axis "bloch" / "periodic" / "pec" -> BoundarySpec"""
    make = {"bloch": lambda a: td.Boundary.bloch(bloch[a]), "periodic": lambda a: td.Boundary.periodic(), "pec": lambda a: td.Boundary.pec()}
    return td.BoundarySpec(**{AX[a]: make[kinds[a]](a) for a in range(3)})


def corner_cell(N, kinds, center=(0.0, 0.0, 0.0), radius=0.18, run_time=1e-12):
    """``test_aniso_bloch.wrapped_cell`` with a say in every axis: a cell of N cells of DL whose biaxial sphere sits on the lattice point at
    the corner of every axis that is not walled (its images on the other corners complete it), a lossy box and two dipoles where the
    window moved by half a period (``center``) holds them as well."""
    size = tuple(n * DL for n in N)
    open_ = [k != "pec" for k in kinds]
    corners = [[-1, 1] if o else [None] for o in open_]
    spheres = [td.Structure(geometry=td.Sphere(center=tuple(0.0 if s is None else s * 0.5 * size[a] for a, s in enumerate((sx, sy, sz))), radius=radius),
                            medium=tab.BIAXIAL) for sx in corners[0] for sy in corners[1] for sz in corners[2]]
    box = td.Structure(geometry=td.Box(center=(0.25, 0.05, 0.12 if open_[2] else 0.0), size=(0.11, 0.07, 0.19)),
                       medium=td.Medium(permittivity=2.5, conductivity=0.02))
    return td.Simulation(size=size, center=center, grid_spec=td.GridSpec.uniform(dl=DL), run_time=run_time, subpixel=False,
                         structures=spheres + [box], shutoff=0,
                         sources=[td.PointDipole(center=(0.12, 0.07, 0.03), source_time=tab.PULSE, polarization="Ez"),
                                  td.PointDipole(center=(0.07, 0.2, 0.06 if open_[2] else -0.06), source_time=tab.PULSE, polarization="Hx")],
                         boundary_spec=_faces(kinds))


def live_wraps(spec):
    """[m, 3]: the periods crossed by every slot the kernels read (a node, a weight) and that crosses any"""
    w = np.concatenate([np.asarray(st.nbr_wrap, np.int64)[(st.g != 0) & (st.nbr_ijk[:, :, 0] >= 0)] for st in spec.aniso])
    return w[w.any(axis=1)]


def sign_sets(spec):
    """-> (the single-axis crossings, the two-axis crossings) among the live slots, as sets of ((axis, sign), ...)"""
    one, two = set(), set()
    for w in np.unique(live_wraps(spec), axis=0):
        key = tuple((a, int(w[a])) for a in range(3) if w[a])
        assert len(key) <= 2, w                            # a slot spans two axes at most
        (one if len(key) == 1 else two).add(key)
    return one, two


# the stencil of spec.AnisoSet: E_a at (i_a, i_b) reads E_b at {i_a, i_a + 1} x {i_b - 1, i_b} — along its own axis a slot can leave the cell
# by +1 only, along the other by -1 only.  Every axis has both signs among the single crossings (+a from list a, -a from the other two),
# and a slot across two axes is (+a, -b) for each ordered pair: six of the twelve sign pairs.  (+a, +b) and (-a, -b) are in no list.
SINGLE = {((a, s),) for a in range(3) for s in (1, -1)}
PAIRS = {tuple(sorted(((a, 1), (b, -1)))) for a in range(3) for b in range(3) if a != b}


# ---------------------------------------------------------------------------------------------------------------- scenarios
def bloch_xy_corner():
    """18 x 14 x 10, ``wrapped_cell`` as it is: Bloch x / y, PEC z, the sphere on the corner lattice point"""
    spec = _spec(tab.wrapped_cell())
    one, two = sign_sets(spec)
    assert spec.shape == (18, 14, 10) and {k for k in SINGLE if k[0][0] < 2} <= one and {k for k in PAIRS if all(a < 2 for a, _ in k)} <= two
    return spec


def bloch_xyz_corner(center=(0.0, 0.0, 0.0)):
    """16 x 14 x 10, Bloch phases on all three axes, the sphere on the corner of the cell: slots across z and across each pair of axes"""
    spec = _spec(corner_cell((16, 14, 10), ("bloch",) * 3, center))
    assert spec.shape == (16, 14, 10) and len(set(np.abs(spec.bloch))) == 3 and np.abs(spec.bloch).min() >= 0.2
    return spec


def bloch_clear_pml_z():
    """``clear_case("pml")``: the wrap array present, every code 0; CPML on z"""
    spec = _spec(tab.clear_case("pml"))
    assert all(st.nbr_wrap is not None and not np.abs(st.nbr_wrap[st.g != 0]).any() for st in spec.aniso) and spec.pml[2][0].num_layers == 3
    return spec


def periodic_xyz_corner():
    """18 x 14 x 10, plain periodic faces on all three axes, the sphere on the corner: real fields reading far-side nodes"""
    spec = _spec(corner_cell((18, 14, 10), ("periodic",) * 3))
    one, _ = sign_sets(spec)
    assert spec.shape == (18, 14, 10) and spec.bloch is None and one == SINGLE
    return spec


def bloch_seam_bar():
    """264 x 8 x 12, Bloch x / y, PEC z: an anisotropic bar from cell 244 to cell 262, through the cell in y — across the x-tile seam of
    the device layout (rows of 266 cells and their padding, every node moved by the ghost cells) and across the y wrap"""
    sim = mc._box_sim((264, 8, 12), _faces(("bloch", "bloch", "pec")))
    b = np.asarray(discretize(sim, n_steps=1).spec.boundaries[0])
    x0, x1 = float(b[244]), float(b[262])
    bar = td.Structure(geometry=td.Box(center=(0.5 * (x0 + x1), 0.0, 0.03), size=(x1 - x0, td.inf, 0.3)), medium=tab.BIAXIAL)
    spec = _spec(dataclasses.replace(sim, structures=[bar]))
    ii = np.concatenate([s.ijk[:, 0] for s in spec.aniso])
    assert spec.shape == (264, 8, 12) and ii.min() < ds.X_TILE - 3 and ii.max() >= ds.X_TILE + 2, (ii.min(), ii.max())
    assert live_wraps(spec)[:, 1].any() and all(p != 0.0 for p in spec.bloch[:2])
    return spec


def small_at_wall():
    """12 x 12 x 12, Bloch x / y, PEC z: two bodies of 2 x 2 x 2 cells, one on the z- wall — its E_z nodes of the first cell read the pinned
    E_x / E_y nodes on the wall, which are in no list — and one under the z+ wall: its E_z nodes of the last cell reach beyond it and have
    empty slots.  (Both on the wall, neither moved in: no listed node is a pinned one.)"""
    bodies = [td.Structure(geometry=td.Box(center=(x * DL, y * DL, z * DL), size=(2 * DL,) * 3), medium=tab.BIAXIAL)
              for x, y, z in ((-2.0, -1.0, -5.0), (3.0, 2.0, 5.0))]
    spec = _spec(mc._box_sim((12, 12, 12), _faces(("bloch", "bloch", "pec")), bodies))
    assert spec.shape == (12, 12, 12) and max(len(s.ijk) for s in spec.aniso) < 64
    return spec


SCENARIOS = {"bloch_xy_corner": bloch_xy_corner, "bloch_xyz_corner": bloch_xyz_corner, "bloch_clear_pml_z": bloch_clear_pml_z,
             "periodic_xyz_corner": periodic_xyz_corner, "bloch_seam_bar": bloch_seam_bar, "small_at_wall": small_at_wall}


def sign_name(w):
    return "".join(f"{'+' if w[a] > 0 else '-'}{AX[a]}" for a in range(3) if w[a])


class Scenario(lc.Scenario):
    """the reference is the oracle itself; a slot of weight zero is an empty one, as the kernels see it"""
    ATTR, TAG, ORACLE, SCENARIOS = "aniso", "aniso", OracleFdtd, SCENARIOS

    def slots_of(self, s):
        return np.where((np.asarray(s.g) != 0)[:, :, None], np.asarray(s.nbr_ijk), -1), True

    def wraps_of(self, s, e):
        """the signs of the slots of entry e that cross a wrap, in words"""
        w = np.asarray(s.nbr_wrap, np.int64)[e][self.slots_of(s)[0][e, :, 0] >= 0]
        w = w[w.any(axis=1)]
        return f" ({', '.join(sign_name(v) for v in w)})" if len(w) else ""


def scenario(label):
    return lc.scenario(Scenario, label)


def check_scenario(lib, label, K, what=""):
    """both paths in single steps, every node under the bar of (scenario, K).  -> {path: (worst node, run)}"""
    sc, out = scenario(label), {}
    for p in PATHS:
        got = sc.run(lib, K, p)
        assert got.pairs == 0 and got.shell2_pairs == 0, (label, K, p, got.pairs)          # single steps only
        out[p] = (sc.check_nodes(got.fields, K, what + p), got)
    return out


# ---------------------------------------------------------------------------------------------------------------- the oracle's own pin
def oracle_translation(cell, n_steps=150, dtype=np.float64):
    """``cell(center)`` -> Simulation.  The fp64 oracle of the corner cell A and of the same cell with its window moved by half a period
    along every periodic axis (B: the body in the middle, no slot crosses, the phase factor of the coupling is never formed), B mapped
    back onto A's cells as ``test_aniso_bloch.translated_fields`` maps it: A's cell i holds B's cell i - s, times exp(-i phi) where that
    cell lies one period back.  -> (A's fields, B's mapped, A's spec)"""
    spec_a = discretize(cell((0.0, 0.0, 0.0)), n_steps=n_steps).spec
    shift = [n // 2 if spec_a.bloch[a] != 0.0 else 0 for a, n in enumerate(spec_a.shape)]
    spec_b = discretize(cell(tuple(s * DL for s in shift)), n_steps=n_steps).spec
    assert len(live_wraps(spec_a)) and not len(live_wraps(spec_b)) and spec_b.shape == spec_a.shape
    assert [len(st.ijk) for st in spec_a.aniso] == [len(st.ijk) for st in spec_b.aniso]
    out = []
    for spec in (spec_a, spec_b):
        o = OracleFdtd(spec, dtype=dtype)
        o.run()
        out.append([np.array(f) for f in o.E + o.H])
    mapped = []
    for f in out[1]:
        g = np.roll(f, tuple(shift[::-1]), axis=(0, 1, 2))
        for a in range(3):
            if shift[a]:
                sl = [slice(None)] * 3
                sl[2 - a] = slice(0, shift[a])
                g[tuple(sl)] *= np.exp(-1j * spec_a.bloch[a])
        mapped.append(g)
    return out[0], mapped, spec_a


def node_agreement(fa, mapped):
    """per component the largest |A - B mapped| over the largest |A| of that component"""
    return [float(np.abs(fa[c] - mapped[c]).max() / np.abs(fa[c]).max()) for c in range(6)]


# ---------------------------------------------------------------------------------------------------------------- planted deviations
def curls(sc):
    """per E component the curl term the first step applied at every node, recovered as the coupling recovers it — (E^1 - Ca E^0) / Cb, 0 on
    PEC nodes — from the fp64 run WITHOUT the lists (its E after one step is the unpatched one): the reference alone"""
    o, new = OracleFdtd(sc.plain), sc.ref_plain(1)
    out = []
    for b in range(3):
        ca, cb = np.broadcast_to(o.ca[b], new[b].shape), np.broadcast_to(o.cb[b], new[b].shape)
        out.append(np.where(cb == 0, 0.0, (new[b] - ca * sc.state[b]) / np.where(cb == 0, 1.0, cb)))
    return out


def slot_terms(sc, s, nbr=None):
    """[n, 8] complex: what each slot of list ``s`` (read at ``nbr`` instead of its own nodes) adds to its node in the first step,
    (dt / eps0) g curl_b(j) exp(i theta), and theta [n, 8] = sum_a s_a phi_a"""
    from oracle.fdtd_numpy import _EPS0
    nbr = sc.slots_of(s)[0] if nbr is None else nbr
    phases = np.asarray(sc.spec.bloch, np.float64) if sc.spec.bloch is not None else np.zeros(3)
    theta = np.asarray(s.nbr_wrap, np.int64) @ phases
    t, curl = np.zeros(nbr.shape[:2], complex), curls(sc)
    for slot in range(8):
        ok = nbr[:, slot, 0] >= 0
        t[ok, slot] = (sc.spec.dt / _EPS0) * s.g[ok, slot] * lc.value_at(curl, s.nbr_comp[slot], nbr[ok, slot]) * np.exp(1j * theta[ok, slot])
    return t, theta


def with_wrap(s, e, slot, w):
    """{nbr_wrap: the periods slot ``slot`` of entry e crossed set to ``w``}"""
    wrap = np.array(s.nbr_wrap)
    wrap[e, slot] = w
    return {"nbr_wrap": wrap}


def without_last(s):
    return {name: np.ascontiguousarray(getattr(s, name)[:-1]) for name in ("ijk", "nbr_ijk", "g", "nbr_wrap")}
