"""Scenes of the device rasteriser (``fdtd_rasterize``, csrc/fdtd_raster.hpp; tests/test_emu_raster.py, tests/test_gpu_raster.py).
The host path of ``discretize.rasterize`` is the exact reference: every check is array equality of ``spec.mat_idx`` (uint16) and
entry-for-entry equality of ``spec.media``.  The grids are a few thousand nodes: what can go wrong is about faces, roundings, the
order of overwrites and the launch tiles (64 x nodes by 4 rows), not about size.

Two scenes exist to tell a wrong build from the right one (docs/history/DEVICE_RASTER.md records the planted runs):
  * ``scene_boxes``: the box ``on_lines`` has its faces on grid lines — a node with |x - x0| == L / 2 exactly (``nodes_on_faces``
    counts them): ``<`` in place of ``<=`` loses them;
  * ``scene_spheres_graded`` / ``scene_cylinders``: ``touching_sphere`` / ``touching_cylinder`` put a surface through a node of the
    graded grid whose squared distance changes when a product and a sum are contracted into one FMA (``contraction_changes``
    evaluates both forms in exact rational arithmetic).  The emulator library built with -ffp-contract=fast loses the sphere's node
    (Ey node (23, 13, 9)); it fuses the cylinder's two-term sum the other way round and keeps that node, so the sphere is the
    scene that tells the builds apart.
"""
import dataclasses
from fractions import Fraction

import numpy as np

import tidy3d_amd.schema as td
from tidy3d_amd.discretize import discretize, make_boundaries

PULSE = td.GaussianPulse(freq0=3e14, fwidth=1.5e14)
PEC_WALLS = td.BoundarySpec.all_sides(td.PECBoundary())


def graded(n: int, d0: float, ratio: float = 1.06):
    """n steps that grow from both ends towards the middle: a graded axis, no two neighbouring steps alike"""
    return tuple(d0 * ratio ** min(i, n - 1 - i) * (1.0 + 0.013 * (i % 3)) for i in range(n))


X37, Y21, Z13 = graded(37, 0.031), graded(21, 0.043), graded(13, 0.052)


def base(steps=(X37, Y21, Z13), structures=(), **kw):
    grids = [td.UniformGrid(dl=s[1]) if s[0] == "uniform" else td.CustomGrid(dl=s) for s in steps]
    size = tuple(s[1] * s[2] if s[0] == "uniform" else float(sum(s)) for s in steps)
    kw.setdefault("boundary_spec", PEC_WALLS)
    kw.setdefault("subpixel", False)          # the staircase itself; scene 6 switches the averaging on
    kw.setdefault("sources", [td.PointDipole(center=(0.0, 0.0, 0.0), source_time=PULSE, polarization="Ez")])
    return td.Simulation(size=size, grid_spec=td.GridSpec(grid_x=grids[0], grid_y=grids[1], grid_z=grids[2]), run_time=1e-13,
                         structures=list(structures), shutoff=0, **kw)


def lines(steps=(X37, Y21, Z13)):
    """the cell boundaries of ``base(steps)`` per axis"""
    return [np.asarray(b, float) for b in make_boundaries(base(steps))]


def box(medium, center, size, name=None):
    return td.Structure(geometry=td.Box(center=tuple(center), size=tuple(size)), medium=medium, name=name)


def between(b, i, j):
    """centre and size of the interval between grid lines i and j, formed as a user (or AutoGrid's snapping) would: the faces
    centre -+ size / 2 are the lines, or one rounding off them"""
    return 0.5 * (b[i] + b[j]), b[j] - b[i]


def overlapping():
    bx, by, bz = lines()
    return [box(td.Medium(permittivity=2.0), (bx[14], by[9], bz[6]), (0.5, 0.4, 0.3), "a"),
            box(td.Medium(permittivity=3.0), (bx[17] + 0.01, by[11], bz[7]), (0.45, 0.35, 0.25), "b"),
            box(td.Medium(permittivity=4.0, conductivity=0.1), (bx[20], by[8] - 0.02, bz[5]), (0.4, 0.5, 0.2), "c")]


def scene_boxes(reverse: bool = False):
    """37 x 21 x 13, graded: three overlapping boxes (in either order), a PEC box, a box with its faces on grid lines, a box infinite
    along z, a box wholly outside the domain, a box one node thick"""
    bx, by, bz = lines()
    three = overlapping()
    cx, sx = between(bx, 5, 12)
    cy, sy = between(by, 3, 17)
    cz, sz = between(bz, 2, 9)
    rest = [box(td.PECMedium(), (bx[30], by[15], bz[9]), (0.2, 0.3, 0.25), "pec"),
            box(td.Medium(permittivity=5.0), (cx, cy, cz), (sx, sy, sz), "on_lines"),
            box(td.Medium(permittivity=6.0), (bx[26], by[5], 0.0), (0.12, 0.2, td.inf), "inf_z"),
            box(td.Medium(permittivity=7.0), (50.0, 0.0, 0.0), (0.5, 0.5, 0.5), "outside"),
            box(td.Medium(permittivity=8.0), (bx[33], 0.0, 0.0), (1e-3, 0.5, 0.4), "one_node")]
    return base(structures=(three[::-1] if reverse else three) + rest)


def nodes_on_faces(sim, name="on_lines"):
    """how many nodes, over the three components and axes, lie on a face of the box exactly: |p - p0| == L / 2 in fp64"""
    geo = next(s.geometry for s in sim.structures if s.name == name)
    spec = discretize(dataclasses.replace(sim, structures=[]), n_steps=2).spec
    return sum(int(np.sum(np.abs(np.asarray(spec.yee_coords(c)[a], float) - geo.center[a]) == geo.size[a] / 2))
               for c in range(3) for a in range(3))


def scene_autogrid():
    """AutoGrid on every axis: the mesher snaps grid lines to the faces of the box (the case tests/test_fuzz_frontend.py found)"""
    body = box(td.Medium(permittivity=6.25), (0.013, -0.021, 0.007), (0.37, 0.29, 0.23), "snapped")
    return td.Simulation(size=(1.2, 1.0, 0.9), grid_spec=td.GridSpec.auto(wavelength=0.6, min_steps_per_wvl=12), run_time=1e-13,
                         structures=[body, box(td.Medium(permittivity=2.0), (0.3, 0.2, 0.0), (0.3, 0.3, 0.3), "second")],
                         sources=[td.PointDipole(center=(-0.4, 0, 0), source_time=PULSE, polarization="Ez")],
                         boundary_spec=PEC_WALLS, shutoff=0, subpixel=False)


# ---- spheres ------------------------------------------------------------------------------------------------------------------
DL = 0.0625                        # a power of two: the nodes of the uniform axes and their differences are exact
U_STEPS = (("uniform", DL, 24), ("uniform", DL, 20), ("uniform", DL, 16))


def _sq_sum(terms, contract):
    """(d0^2 + d1^2) + d2^2 with one rounding per operation — or, ``contract``, the form clang's -ffp-contract=fast gives: the first
    sum takes d0^2 unrounded (fma(d0, d0, d1^2)), every further sum its new product (fma(d2, d2, sum))"""
    sq = [Fraction(t) ** 2 for t in terms]
    if not contract:
        acc = float(sq[0])
        for s in sq[1:]:
            acc = float(Fraction(acc) + Fraction(float(s)))
        return acc
    acc = float(sq[0] + Fraction(float(sq[1])))
    for s in sq[2:]:
        acc = float(Fraction(acc) + s)
    return acc


def contraction_changes(coords, center, axes=(0, 1, 2)):
    """the first node (i, j, k) of a component's coordinates whose squared distance from ``center`` over ``axes`` differs between the
    two forms, with both values"""
    for k, z in enumerate(coords[2]):
        for j, y in enumerate(coords[1]):
            for i, x in enumerate(coords[0]):
                d = [float(p) - float(c) for p, c in zip((x, y, z), center)]
                d = [d[a] for a in axes]
                plain, fused = _sq_sum(d, False), _sq_sum(d, True)
                if plain != fused:
                    return (i, j, k), plain, fused
    return None


def touching_radius(plain, fused):
    """a radius whose square — as Python's ``radius ** 2`` and as r * r — lies between the two squared distances, the larger included:
    the node is inside by one form and outside by the other"""
    lo, hi = min(plain, fused), max(plain, fused)
    r = float(np.sqrt(lo))
    for _ in range(64):
        if lo <= r ** 2 < hi and lo <= r * r < hi:
            return r
        r = float(np.nextafter(r, np.inf if r ** 2 < lo else -np.inf))
    return None


def touching(component, center, axes=(0, 1, 2), steps=(X37, Y21, Z13)):
    """(radius, node, plain, fused) of a surface around ``center`` through a node of E component ``component`` on which contraction
    decides; searched in exact arithmetic, so the scene is the same on every machine"""
    spec = discretize(base(steps), n_steps=2).spec
    coords = [np.asarray(v, float) for v in spec.yee_coords(component)]
    first = [len(c) // 2 + 3 if a in axes else 0 for a, c in enumerate(coords)]        # (a few cells from the centre: a small body)
    sub = [c[first[a]:] if a in axes else c[:1] for a, c in enumerate(coords)]
    for shift in range(40):
        cen = tuple(c + 1e-3 * shift for c in center)
        hit = contraction_changes(sub, cen, axes)
        if hit is not None:
            r = touching_radius(hit[1], hit[2])
            if r is not None:
                return cen, r, tuple(n + f for n, f in zip(hit[0], first)), hit[1], hit[2]
    raise AssertionError("no node found on which contraction decides")


def scene_spheres():
    """24 x 20 x 16, uniform (dl = 2^-4): a sphere centred on an Ez node whose surface passes through nodes exactly (radius 5 dl: the
    axis points and the 3-4-5 triples)"""
    exact = td.Structure(geometry=td.Sphere(center=(0.0, 0.0, DL / 2), radius=5 * DL), medium=td.Medium(permittivity=3.0), name="exact")
    return base(U_STEPS, [exact])


def scene_spheres_graded():
    """graded 37 x 21 x 13: the touching sphere (first: the later ones leave its node alone), a sphere off-centre, a sphere cut by the
    domain wall"""
    bx, by, bz = lines()
    cen, r, _, _, _ = touching(1, (0.0931, -0.0517, 0.0233))
    return base(structures=[
        td.Structure(geometry=td.Sphere(center=cen, radius=r), medium=td.Medium(permittivity=9.0), name="touching_sphere"),
        td.Structure(geometry=td.Sphere(center=(-0.213, -0.171, 0.037), radius=0.171), medium=td.Medium(permittivity=3.0), name="off_centre"),
        td.Structure(geometry=td.Sphere(center=(bx[-1] - 0.05, by[0] + 0.1, 0.05), radius=0.3), medium=td.Medium(permittivity=4.5), name="cut")])


# ---- cylinders ----------------------------------------------------------------------------------------------------------------
DISPERSIVE = td.Lorentz(eps_inf=2.0, coeffs=[(1.5, 4e14, 3e13)])
DIAGONAL = td.AnisotropicMedium(xx=td.Medium(permittivity=2.0), yy=td.Medium(permittivity=3.0), zz=td.Medium(permittivity=4.0, conductivity=0.05))


def scene_cylinders():
    """graded 37 x 21 x 13: cylinders along x (a diagonal AnisotropicMedium: one index per component), y (infinite length, a dispersive
    medium) and z (its end caps on grid lines), and one along z through a node on which contraction decides"""
    bx, by, bz = lines()
    cz, lz = between(bz, 3, 10)
    cen, r, _, _, _ = touching(2, (-0.2071, 0.1113, 0.0), axes=(0, 1))
    cyl = lambda axis, center, radius, length, med, name: td.Structure(                     # noqa: E731
        geometry=td.Cylinder(axis=axis, center=center, radius=radius, length=length), medium=med, name=name)
    return base(structures=[cyl(2, (cen[0], cen[1], 0.0), r, 0.3, td.Medium(permittivity=9.0), "touching_cylinder"),
                            cyl(0, (0.05, -0.1, 0.02), 0.17, 0.6, DIAGONAL, "along_x"),
                            cyl(1, (0.3, 0.0, -0.05), 0.21, td.inf, DISPERSIVE, "along_y"),
                            cyl(2, (-0.31, 0.09, cz), 0.19, lz, td.Medium(permittivity=5.0), "caps_on_lines")])


# ---- two x tiles --------------------------------------------------------------------------------------------------------------
def scene_two_tiles():
    """264 x 8 x 12, uniform: a box across index 256 (the seam of two 256-cell x tiles of the sweep; here also the fifth 64-node
    tile of a launch) and a sphere on it"""
    dl = 0.0625
    x256 = -132 * dl + 256 * dl
    return base((("uniform", dl, 264), ("uniform", dl, 8), ("uniform", dl, 12)), [box(td.Medium(permittivity=2.5), (x256, 0.0, 0.0), (0.62, 0.2, 0.3), "across"),
                                                 td.Structure(geometry=td.Sphere(center=(x256, 0.03, -0.02), radius=0.17),
                                                              medium=td.Medium(permittivity=6.0), name="on_seam")])


# ---- fallbacks ----------------------------------------------------------------------------------------------------------------
def fallback_scenes():
    """scene_boxes plus one structure the device rasteriser does not take -> (simulation, the words of the log line)"""
    sim = scene_boxes()
    slab = td.Structure(geometry=td.PolySlab(vertices=[(-0.2, -0.1), (0.2, -0.1), (0.0, 0.2)], axis=2, slab_bounds=(-0.1, 0.1)),
                        medium=td.Medium(permittivity=2.2), name="slab")
    sheet = td.Structure(geometry=td.Box(center=(0.0, 0.0, 0.0), size=(0.4, 0.3, 0.0)),
                         medium=td.Medium2D(ss=td.Medium(conductivity=2e-3), tt=td.Medium(conductivity=2e-3)), name="sheet")
    kerr = box(td.Medium(permittivity=2.0, nonlinear_spec=td.NonlinearSpec(models=[td.NonlinearSusceptibility(chi3=1e-3)], num_iters=3)),
               (0.1, 0.0, 0.0), (0.2, 0.2, 0.2), "kerr")
    add = lambda st: dataclasses.replace(sim, structures=list(sim.structures) + [st])       # noqa: E731
    return {"polyslab": (add(slab), "structure 8 'slab' holds geometry 'PolySlab'"),
            "medium2d": (add(sheet), "structure 8 'sheet' holds a Medium2D sheet"),
            "kerr": (add(kerr), "structure 8 'kerr' holds a fully anisotropic, time-modulated or nonlinear medium")}


# ---- the checks ---------------------------------------------------------------------------------------------------------------
_HOST = {}


def host_spec(key, sim, **kw):
    """the host path's SolverSpec of a scene, computed once per session and left unchanged"""
    if key not in _HOST:
        _HOST[key] = discretize(sim, n_steps=4, rasterize_device=False, **kw).spec
    return _HOST[key]


def same_raster(a, b):
    assert a.mat_idx.dtype == b.mat_idx.dtype == np.uint16 and a.mat_idx.shape == b.mat_idx.shape
    bad = np.argwhere(a.mat_idx != b.mat_idx)
    assert bad.size == 0, "%d nodes differ, the first: component, k, j, i = %s: %d against %d" % (
        len(bad), tuple(bad[0]), a.mat_idx[tuple(bad[0])], b.mat_idx[tuple(bad[0])])
    assert len(a.media) == len(b.media) and all(x == y for x, y in zip(a.media, b.media))


def check_scene(lib, key, sim, shape=None, launches=None, **kw):
    """``rasterize_device=True`` against the host path: equal indices, equal tables, the log line"""
    host = host_spec(key, sim, **kw)
    dev = discretize(sim, n_steps=4, rasterize_device=True, lib=lib, **kw).spec
    if shape is not None:
        assert tuple(dev.shape) == shape, dev.shape
    same_raster(dev, host)
    n = len(sim.all_structures)
    assert host.raster_log == f"Rasterised {n} structures: host."
    assert dev.raster_log.startswith(f"Rasterised {n} structures: device (") and dev.raster_log.endswith(" launches).")
    if launches is not None:
        assert dev.raster_log == f"Rasterised {n} structures: device ({launches} launches)."
    return dev, host
