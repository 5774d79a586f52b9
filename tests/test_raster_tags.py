"""The tag volumes of `discretize.rasterize` — which fully anisotropic, time-modulated or Kerr medium a node belongs to — seen through
the node lists they end in (spec.aniso / spec.modulation / spec.nonlinear): a later body takes the nodes over whichever branch
paints it, the nodes the sweep holds at zero are in no list, and the refusals keep their words.  Grids of 12 x 10 x 8 cells, no engine."""
import itertools

import numpy as np
import pytest

import tidy3d_amd.schema as td
from tidy3d_amd.data import DataArray
from tidy3d_amd.discretize import discretize
from tidy3d_amd.exceptions import Tidy3dNotImplementedError
from tidy3d_amd.spec import BC_PEC, BC_PERIODIC

N = (12, 10, 8)
DL = 0.05
PULSE = td.GaussianPulse(freq0=3e14, fwidth=1.5e14)
PEC = td.Boundary(minus=td.PECBoundary(), plus=td.PECBoundary())
KINDS = ("aniso", "modulation", "nonlinear")
_SLOT_OFFSETS = ((0, -1), (1, -1), (0, 0), (1, 0))          # (along a, along b) of the four E_b nodes around an E_a node


def fully_anisotropic(k=0):
    return td.FullyAnisotropicMedium(permittivity=[[2.5 + 0.01 * k, 0.3, 0.0], [0.3, 2.2, 0.1], [0.0, 0.1, 2.0]])


def modulated(k=0):
    stm = td.SpaceTimeModulation(time_modulation=td.ContinuousWaveTimeModulation(freq0=1e15, amplitude=0.5, phase=0.3))
    return td.Medium(permittivity=3.0 + 0.01 * k, modulation_spec=td.ModulationSpec(permittivity=stm))


def kerr(k=0):
    return td.Medium(permittivity=3.0, nonlinear_spec=td.NonlinearSpec(models=(td.NonlinearSusceptibility(chi3=1e-3 * (1 + k)),), num_iters=5))


MEDIUM = {"aniso": fully_anisotropic, "modulation": modulated, "nonlinear": kerr}


def custom_medium():
    x = np.array([-0.3, 0.3])
    a = DataArray(np.array([2.0, 4.0])[:, None, None] * np.ones((1, 2, 2)), {"x": x, "y": np.array([-9.0, 9.0]), "z": np.array([-9.0, 9.0])})
    a.tag = "SpatialDataArray"
    return td.CustomMedium(permittivity=a, interp_method="nearest")


def sim(structures, bspec=None, **kw):
    grid = td.GridSpec(grid_x=td.CustomGrid(dl=(DL,) * N[0]), grid_y=td.CustomGrid(dl=(DL,) * N[1]), grid_z=td.CustomGrid(dl=(DL,) * N[2]))
    return td.Simulation(size=tuple(float(np.sum((DL,) * n)) for n in N), grid_spec=grid, run_time=1e-13, structures=list(structures), subpixel=False,
                         sources=[td.PointDipole(center=(0.03, -0.07, 0.01), source_time=PULSE, polarization="Ez")], monitors=[],
                         boundary_spec=bspec or td.BoundarySpec(x=PEC, y=PEC, z=PEC), shutoff=0, **kw)


def spec_of(structures, bspec=None, **kw):
    spec = discretize(sim(structures, bspec, **kw), n_steps=2).spec
    assert spec.shape == N
    return spec


def listed(spec, kind):
    """the listed nodes as a boolean [3, nx, ny, nz]"""
    out = np.zeros((3,) + N, bool)
    for s in getattr(spec, kind):
        assert not out[s.comp][s.ijk[:, 0], s.ijk[:, 1], s.ijk[:, 2]].any()          # each node at most once
        out[s.comp][s.ijk[:, 0], s.ijk[:, 1], s.ijk[:, 2]] = True
    return out


def inside(spec, geo):
    """`geo.inside` at the Yee coordinates of the three E components, [3, nx, ny, nz]"""
    return np.stack([np.asarray(geo.inside(*np.meshgrid(*spec.yee_coords(c), indexing="ij")), bool) for c in range(3)])


def held_at_zero(spec):
    """nodes the sweep holds at zero: PEC cells, and E tangential to a PEC min wall (index 0 along the wall's axis)"""
    out = spec.mat_idx.transpose(0, 3, 2, 1) == 0
    for c, ax in itertools.product(range(3), range(3)):
        if ax != c and spec.bc[ax][0] == BC_PEC:
            sl = [slice(None)] * 3
            sl[ax] = 0
            out[c][tuple(sl)] = True
    return out


def coupled_rows(spec, body):
    """rows of the coupling lists of fully anisotropic bodies whose nodes are ``body`` [3, nx, ny, nz]: the nodes themselves and every
    E_a node with one of its eight neighbour slots inside (no neighbour beyond a wall that is not periodic)"""
    out = body.copy()
    for a in range(3):
        for b in ((a + 1) % 3, (a + 2) % 3):
            for da, db in _SLOT_OFFSETS:
                for ijk in np.argwhere(body[b]):
                    row = ijk.copy()
                    row[a] -= da
                    row[b] -= db
                    ok = True
                    for ax in (a, b):
                        if spec.bc[ax][0] == BC_PERIODIC:
                            row[ax] %= N[ax]
                        elif not 0 <= row[ax] < N[ax]:
                            ok = False
                    if ok:
                        out[a][tuple(row)] = True
    return out


# faces and centres off the grid lines and off the cell centres: no node within a rounding of a surface
TAGGED = {"box": td.Box(center=(-0.053, 0.011, 0.007), size=(0.31, 0.27, 0.23)), "sphere": td.Sphere(center=(-0.053, 0.011, 0.007), radius=0.151)}
LATER = {"box": (td.Box(center=(0.093, 0.047, 0.021), size=(0.21, 0.19, 0.17)), None),
         "sphere": (td.Sphere(center=(0.093, 0.047, 0.021), radius=0.117), None),
         "custom": (td.Box(center=(0.093, 0.047, 0.021), size=(0.21, 0.19, 0.17)), custom_medium)}


@pytest.mark.parametrize("earlier", list(TAGGED))
@pytest.mark.parametrize("later", list(LATER))
@pytest.mark.parametrize("kind", KINDS)
def test_a_later_body_takes_the_nodes_over(kind, later, earlier):
    geo, (geo2, med2) = TAGGED[earlier], LATER[later]
    med2 = med2() if med2 else td.Medium(permittivity=2.0)
    spec = spec_of([td.Structure(geometry=geo, medium=MEDIUM[kind]()), td.Structure(geometry=geo2, medium=med2)])
    got = listed(spec, kind)
    body, covered = inside(spec, geo), inside(spec, geo2)
    assert (body & covered).any() and (body & ~covered).any() and (covered & ~body).any()
    want = body & ~covered
    if kind == "aniso":
        want = coupled_rows(spec, want)
        assert (want & covered).any()                   # rows under the later body that couple into what is left of the tagged one
    else:
        assert not (got & covered).any()
    want &= ~held_at_zero(spec)
    assert np.array_equal(got, want), (int(got.sum()), int(want.sum()))
    # the later body alone leaves no list; the tagged body alone holds the covered nodes too
    assert not getattr(spec_of([td.Structure(geometry=geo2, medium=med2)]), kind)
    alone = listed(spec_of([td.Structure(geometry=geo, medium=MEDIUM[kind]())]), kind)
    assert (alone & covered & body).any()


@pytest.mark.parametrize("axis", range(3))
@pytest.mark.parametrize("kind", KINDS)
def test_no_list_holds_a_node_the_sweep_holds_at_zero(kind, axis):
    """a body that fills the domain, a PEC min wall on one axis (the others periodic), a PEC box inside it: no tangential node at index 0
    along the wall's axis, no node on a PEC cell — and the nodes beside them are listed"""
    per = td.Boundary.periodic()
    bspec = td.BoundarySpec(**{"xyz"[a]: PEC if a == axis else per for a in range(3)})
    pec_box = td.Box(center=(0.093, 0.047, 0.021), size=(0.21, 0.19, 0.17))
    spec = spec_of([td.Structure(geometry=td.Box(size=(td.inf, td.inf, td.inf)), medium=MEDIUM[kind]()),
                    td.Structure(geometry=pec_box, medium=td.PEC)], bspec)
    got = listed(spec, kind)
    pec = spec.mat_idx.transpose(0, 3, 2, 1) == 0
    assert np.array_equal(pec, inside(spec, pec_box))
    assert not (got & pec).any()
    sl = [slice(None)] * 3
    sl[axis] = 0
    for c in range(3):
        assert got[c][tuple(sl)].any() == (c == axis)           # the normal component on the wall is an unknown
        for a in range(3):
            if a != axis:                                       # index 0 of a periodic axis is a node like any other
                s2 = [slice(None)] * 3
                s2[a] = 0
                assert got[c][tuple(s2)].any()
    want = ~pec & ~held_at_zero(spec)
    assert np.array_equal(got, want)                           # (fully anisotropic: every row outside the box couples or lies inside)


def test_a_pec_sheet_inside_a_fully_anisotropic_body_leaves_no_row_on_its_nodes():
    sheet = td.Structure(geometry=td.Box(center=(-0.053, 0.011, 0.0), size=(0.2, 0.15, 0)), medium=td.Medium2D(ss=td.PEC, tt=td.PEC))
    spec = spec_of([td.Structure(geometry=TAGGED["box"], medium=fully_anisotropic()), sheet])
    got = listed(spec, "aniso")
    pec = spec.mat_idx.transpose(0, 3, 2, 1) == 0
    assert pec[0].any() and pec[1].any() and not pec[2].any() and (pec & inside(spec, TAGGED["box"]) == pec).all()
    assert not (got & pec).any() and got.any()


# ---------------------------------------------------------------------------------------------------------------- refusals
def refused(structures, **kw):
    with pytest.raises(Tidy3dNotImplementedError) as ei:
        discretize(sim(structures, **kw), n_steps=2)
    return str(ei.value)


def _bx(center, size, med):
    return td.Structure(geometry=td.Box(center=center, size=size), medium=med)


PHRASE = {"modulation": "time-modulated (modulation_spec)", "nonlinear": "nonlinear (nonlinear_spec)"}


@pytest.mark.parametrize("kind", ["modulation", "nonlinear"])
def test_a_tagged_component_of_a_composite_medium_is_refused(kind):
    m, plain = MEDIUM[kind](), td.Medium(permittivity=2.0)
    for pos in range(3):
        comps = [plain] * 3
        comps[pos] = m
        got = refused([_bx((0, 0, 0), (0.2, 0.2, 0.2), td.AnisotropicMedium(xx=comps[0], yy=comps[1], zz=comps[2]))])
        assert got == {"modulation": "a time-modulated (modulation_spec) component of 'AnisotropicMedium' is not supported",
                       "nonlinear": "a nonlinear (nonlinear_spec) component of 'AnisotropicMedium' is not supported"}[kind]
    for ss, tt in ((m, plain), (plain, m)):
        got = refused([_bx((0, 0, 0), (0.2, 0.2, 0), td.Medium2D(ss=ss, tt=tt))])
        assert got == {"modulation": "a time-modulated (modulation_spec) component of 'Medium2D' is not supported",
                       "nonlinear": "a nonlinear (nonlinear_spec) component of 'Medium2D' is not supported"}[kind]


@pytest.mark.parametrize("kind", ["modulation", "nonlinear"])
def test_a_sheet_inside_a_tagged_medium_is_refused(kind):
    sheet = _bx((0, 0, 0), (0.2, 0.2, 0), td.Medium2D(ss=td.Medium(conductivity=0.01), tt=td.Medium(conductivity=0.01)))
    body = _bx((0, 0, 0), (0.3, 0.3, 0.3), MEDIUM[kind]())
    assert refused([body, sheet]) == {"modulation": "a Medium2D sheet inside a time-modulated (modulation_spec) medium is not supported",
                                      "nonlinear": "a Medium2D sheet inside a nonlinear (nonlinear_spec) medium is not supported"}[kind]
    # beside the medium, or under it, the sheet is allowed
    assert getattr(spec_of([body, _bx((0.25, 0, 0), (0.05, 0.2, 0), sheet.medium)]), kind)
    assert getattr(spec_of([sheet, body]), kind)
    # a fully anisotropic body takes a sheet
    assert spec_of([_bx((0, 0, 0), (0.3, 0.3, 0.3), fully_anisotropic()), sheet]).aniso


def test_the_kinds_that_do_not_go_together():
    body = {k: _bx((-0.15 + 0.15 * n, 0, 0), (0.1, 0.2, 0.2), MEDIUM[k]()) for n, k in enumerate(KINDS)}
    for order in ((0, 1), (1, 0)):
        pick = lambda a, b: [[body[a], body[b]][i] for i in order]        # noqa: E731
        assert refused(pick("modulation", "aniso")) == "time-modulated (modulation_spec) media together with FullyAnisotropicMedium are not supported"
        assert refused(pick("nonlinear", "aniso")) == "nonlinear (nonlinear_spec) media together with FullyAnisotropicMedium are not supported"
        assert refused(pick("nonlinear", "modulation")) == \
            "nonlinear (nonlinear_spec) media together with time-modulated (modulation_spec) media are not supported"
    # all three: the fully anisotropic body is named first
    assert refused(list(body.values())) == "time-modulated (modulation_spec) media together with FullyAnisotropicMedium are not supported"
    # a fully anisotropic body that a later body covers altogether leaves no list, and nothing to refuse
    cover = _bx((-0.15, 0, 0), (0.1, 0.2, 0.2), td.Medium(permittivity=2.0))
    assert spec_of([body["aniso"], cover, body["nonlinear"]]).nonlinear


# ---------------------------------------------------------------------------------------------------------------- the 254-media limits
def cell_boxes(n, med):
    """n boxes of 1.2 cells, one per cell in index order, each with ``med(k)``"""
    cells = list(itertools.product(range(N[0]), range(N[1]), range(N[2])))[:n]
    return [_bx(tuple((i + 0.5) * DL - 0.5 * N[a] * DL for a, i in enumerate(c)), (1.2 * DL,) * 3, med(k)) for k, c in enumerate(cells)]


@pytest.mark.parametrize("kind,words", [("aniso", "fully anisotropic"), ("modulation", "time-modulated"), ("nonlinear", "nonlinear")])
def test_the_first_refusal_is_at_the_255th_distinct_medium(kind, words):
    assert getattr(spec_of(cell_boxes(254, MEDIUM[kind])), kind)
    assert refused(cell_boxes(255, MEDIUM[kind])) == f"more than 254 distinct {words} media"


def test_how_a_medium_is_found_again():
    """a fully anisotropic medium takes a fresh entry per structure, a time-modulated one is found again by identity, a Kerr one by
    identity or equality"""
    one = {k: MEDIUM[k]() for k in KINDS}
    assert refused(cell_boxes(255, lambda k: one["aniso"])) == "more than 254 distinct fully anisotropic media"
    assert spec_of(cell_boxes(255, lambda k: one["modulation"])).modulation
    assert refused(cell_boxes(255, lambda k: modulated())) == "more than 254 distinct time-modulated media"
    assert spec_of(cell_boxes(255, lambda k: one["nonlinear"])).nonlinear
    spec = spec_of(cell_boxes(255, lambda k: kerr(k % 2)))
    assert len(np.unique(np.concatenate([s.chi3 for s in spec.nonlinear]))) == 2
