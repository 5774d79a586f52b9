"""Digests of what `discretize` returns and of what `HipEngine` hands to the library, scene by scene: run in a worktree of the parent
commit and in this tree, the two outputs are to be identical (docs/history/LIST_SETUP.md).

    python profiles/list_setup/digests.py > profiles/list_setup/digests_here.txt

Per scene one line `name  spec <sha256>  upload <sha256>`.  The spec digest covers every field of the SolverSpec in declaration order
(arrays as dtype, shape, bytes; dataclasses field by field; lists and tuples entry by entry; scalars by repr).  The upload digest covers
the ordered stream of library calls of the engine's set-up on the emulator library: every array given to `engine._ptr` as (dtype, shape,
bytes) and every call name given to `HipEngine._chk`.  A scene that is refused is recorded with the exception's type and text."""
import dataclasses
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
for p in (os.path.join(ROOT, "tests", "hipemu"), os.path.join(ROOT, "tests"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import tidy3d_amd.schema as td                               # noqa: E402
from tidy3d_amd import engine as E                           # noqa: E402
from tidy3d_amd.data import DataArray                        # noqa: E402
from tidy3d_amd.discretize import discretize                 # noqa: E402
from tidy3d_amd.spec import SolverSpec                       # noqa: E402


# ------------------------------------------------------------------------------------------------------------------ hashing
def feed(h, v):
    if isinstance(v, np.ndarray) or isinstance(v, np.generic):
        a = np.ascontiguousarray(v)
        h.update(b"A" + a.dtype.str.encode() + repr(a.shape).encode())
        h.update(a.tobytes())
    elif dataclasses.is_dataclass(v) and not isinstance(v, type):
        h.update(b"D" + type(v).__name__.encode())
        for f in dataclasses.fields(v):
            h.update(f.name.encode())
            feed(h, getattr(v, f.name))
    elif isinstance(v, (list, tuple)):
        h.update(b"L%d" % len(v))
        for x in v:
            feed(h, x)
    elif v is None or isinstance(v, (bool, int, float, complex, str)):
        h.update(b"S" + type(v).__name__.encode() + repr(v).encode())
    else:
        raise TypeError(f"no digest for {type(v)}")


def spec_digest(spec):
    h = hashlib.sha256()
    feed(h, spec)
    return h.hexdigest()


_STREAM = [None]
_ptr0, _chk0 = E._ptr, E.HipEngine._chk


def _ptr(a):
    if _STREAM[0] is not None:
        feed(_STREAM[0], np.asarray(a))
    return _ptr0(a)


def _chk(self, st, what):
    if _STREAM[0] is not None:
        _STREAM[0].update(b"C" + str(what).encode())
    return _chk0(self, st, what)


E._ptr, E.HipEngine._chk = _ptr, _chk
_LIB = []


def emu_lib():
    if not _LIB:
        import build_emu
        from tidy3d_amd.lib import load_library
        _LIB.append(load_library(build_emu.build()))
    return _LIB[0]


def upload_digest(spec, **kw):
    _STREAM[0] = h = hashlib.sha256()
    note = ""
    try:
        with E.HipEngine(spec, lib=emu_lib(), **kw):
            pass
    except Exception as exc:                                 # a refusal is part of the record
        note = f"  engine refused {type(exc).__name__}: {exc}"
        h.update(b"X" + note.encode())
    finally:
        _STREAM[0] = None
    return h.hexdigest() + note


def line(name, make, n_steps=12, **kw):
    """`make` returns a Simulation or a SolverSpec"""
    try:
        got = make()
        spec = got if isinstance(got, SolverSpec) else discretize(got, n_steps=n_steps).spec
    except Exception as exc:
        print(f"{name}  refused {type(exc).__name__}: {exc}", flush=True)
        return
    print(f"{name}  spec {spec_digest(spec)}  upload {upload_digest(spec, **kw)}", flush=True)


# ------------------------------------------------------------------------------------------------------------------ scenes
def _spatial(values, x, y, z):
    a = DataArray(np.asarray(values), {"x": np.asarray(x, float), "y": np.asarray(y, float), "z": np.asarray(z, float)})
    a.tag = "SpatialDataArray"
    return a


def cases_and_scenarios():
    import cases
    import modulation_case
    import nonlinear_case
    import pec_conformal_case
    for name, fn in cases.CASES.items():
        line(f"cases.{name}", fn)
    for mod in (modulation_case, nonlinear_case, pec_conformal_case):
        for name, fn in mod.SCENARIOS.items():
            line(f"{mod.__name__}.{name}", fn)
    # permute_spec: the conformal and the Kerr lists under both axis renamings
    for shift in (1, 2):
        line(f"pec_conformal_case.sphere_blocks.axis_shift{shift}", pec_conformal_case.sphere_blocks, axis_shift=shift)
        line(f"nonlinear_case.pec_box_blocks.axis_shift{shift}", nonlinear_case.pec_box_blocks, axis_shift=shift)
    # the slab-local index form: point sources and TFSF on z-slabs
    for name in ("pec_box", "tfsf_box", "periodic_box"):
        spec = discretize(cases.CASES[name](), n_steps=12).spec
        nz = spec.shape[2]
        cut = nz // 2 + 1
        line(f"cases.{name}.force_comm", lambda: spec, force_comm=True)
        for rank, slab in enumerate(((0, cut), (cut, nz))):
            line(f"cases.{name}.slab{rank}", lambda: spec, slab=slab, rank=rank, n_ranks=2, all_slabs=[(0, cut), (cut, nz)])


def fully_anisotropic():
    import test_fully_anisotropic as t
    from cases import DL, PULSE as P3
    from test_reciprocity import reciprocity_sims
    rot, PULSE = t.rot, t.PULSE
    line("test_fully_anisotropic.body_sim", lambda: t._body_sim().spec)
    # test_wave_plate_matches_the_jones_calculus (its `run` is local: copied)
    med = td.FullyAnisotropicMedium.from_diagonal(1.8 ** 2, 1.5 ** 2, 1.5 ** 2, rot(2, np.pi / 4))
    freqs = np.linspace(1.7e14, 2.3e14, 7)
    per = td.Boundary.periodic()

    def plate(structures, dl=0.02):
        return td.Simulation(size=(4 * dl, 4 * dl, 4.4), grid_spec=td.GridSpec.uniform(dl=dl), run_time=4e-13, structures=structures, subpixel=False,
                             sources=[td.UniformCurrentSource(center=(0, 0, -1.4), size=(td.inf, td.inf, 0), source_time=PULSE, polarization="Ex")],
                             monitors=[td.FieldMonitor(center=(0, 0, 1.3), size=(0, 0, 0), freqs=list(freqs), name="p", fields=["Ex", "Ey"], colocate=False)],
                             boundary_spec=td.BoundarySpec(x=per, y=per, z=td.Boundary.pml(num_layers=12)), shutoff=0)
    line("test_fully_anisotropic.wave_plate.empty", lambda: plate([]))
    line("test_fully_anisotropic.wave_plate.slab",
         lambda: plate([td.Structure(geometry=td.Box(center=(0, 0, 0.3), size=(td.inf, td.inf, 0.6)), medium=med)]))
    # test_reciprocity_and_stability_with_a_fully_anisotropic_body
    med = td.FullyAnisotropicMedium.from_diagonal(2.0, 6.0, 3.0, rot(2, 0.5) @ rot(0, 0.8))
    cfg = dict(N=(20, 18, 16), A=(5, 6, 5), ca=0, B=(14, 11, 10), cb=2,
               bspec=td.BoundarySpec(x=td.Boundary.pml(num_layers=4), y=td.Boundary(minus=td.PMCBoundary(), plus=td.PECBoundary()), z=td.Boundary.periodic()),
               structures=[td.Structure(geometry=td.Box(center=(0.05, 0, 0), size=(0.45, 0.5, 0.4)), medium=med)])
    (d1, _), (d2, _) = reciprocity_sims(n_steps=12, **cfg)
    line("test_fully_anisotropic.reciprocity.1", lambda: d1.spec)
    line("test_fully_anisotropic.reciprocity.2", lambda: d2.spec)
    line("test_fully_anisotropic.stability", lambda: td.Simulation(
        size=(0.8, 0.7, 0.6), grid_spec=td.GridSpec.uniform(dl=0.05), run_time=1e-12, subpixel=False, shutoff=0,
        structures=[td.Structure(geometry=td.Sphere(center=(0.05, 0, 0), radius=0.25), medium=med)],
        sources=[td.PointDipole(center=(-0.2, 0.1, 0.1), source_time=td.GaussianPulse(freq0=3e14, fwidth=1.5e14), polarization="Ez")],
        boundary_spec=td.BoundarySpec.all_sides(td.PECBoundary())))
    # test_what_is_refused
    lossy = td.FullyAnisotropicMedium(permittivity=[[2, 0, 0], [0, 3, 0], [0, 0, 4]], conductivity=[[0.1, 0, 0], [0, 0, 0], [0, 0, 0]])
    line("test_fully_anisotropic.refused.lossy", lambda: td.Simulation(
        size=(1, 1, 1), grid_spec=td.GridSpec.uniform(dl=0.1), run_time=1e-14,
        structures=[td.Structure(geometry=td.Box(size=(0.4, 0.4, 0.4)), medium=lossy)], sources=[td.PointDipole(source_time=PULSE, polarization="Ez")]))
    line("test_fully_anisotropic.refused.force_comm", lambda: t._body_sim().spec, force_comm=True)
    m = td.parse({"type": "FullyAnisotropicMedium", "permittivity": [[2, 0.5, 0], [0.5, 3, 0], [0, 0, 4]]})
    line("test_fully_anisotropic.covered_body", lambda: td.Simulation(
        size=(1, 1, 1), grid_spec=td.GridSpec.uniform(dl=0.1), run_time=1e-14, subpixel=False,
        structures=[td.Structure(geometry=td.Box(size=(0.6, 0.6, 0.6)), medium=m),
                    td.Structure(geometry=td.Box(size=(0.6, 0.6, 0.6)), medium=td.Medium(permittivity=2.0))],
        sources=[td.PointDipole(source_time=PULSE, polarization="Ez")], boundary_spec=td.BoundarySpec.all_sides(td.PECBoundary())))

    # test_random_bodies_fused_two_pass_and_oracle_agree (built inside the test: copied)
    def random_bodies(seed):
        rng = np.random.default_rng(40 + seed)
        N = [int(rng.integers(12, 20)) for _ in range(3)]
        size = tuple(n * DL for n in N)

        def pos():
            return tuple(float(rng.uniform(-0.3, 0.3) * s) for s in size)
        structures = []
        for _ in range(int(rng.integers(1, 4))):
            R = rot(2, float(rng.uniform(0, 3))) @ rot(1, float(rng.uniform(0, 3))) @ rot(0, float(rng.uniform(0, 3)))
            med = td.FullyAnisotropicMedium.from_diagonal(*[float(v) for v in rng.uniform(1.0, 8.0, 3)], R)
            geo = td.Sphere(center=pos(), radius=float(rng.uniform(0.15, 0.3))) if rng.integers(0, 2) else \
                td.Box(center=pos(), size=tuple(float(rng.uniform(0.2, 0.6) * s) for s in size))
            structures.append(td.Structure(geometry=geo, medium=med))
        structures.insert(int(rng.integers(0, len(structures) + 1)),
                          td.Structure(geometry=td.Box(center=pos(), size=tuple(float(rng.uniform(0.2, 0.5) * s) for s in size)),
                                       medium=[td.Medium(permittivity=3.0, conductivity=0.02), td.PEC, td.Lorentz(eps_inf=2.0, coeffs=[(1.5, 4e14, 3e13)])][int(rng.integers(0, 3))]))
        faces = [td.PML(num_layers=3), td.PECBoundary(), td.PMCBoundary(), td.StablePML(num_layers=4)]
        edges = [td.Boundary.periodic() if rng.integers(0, 4) == 0 else
                 td.Boundary(minus=faces[int(rng.integers(0, 4))], plus=faces[int(rng.choice([0, 1, 3]))]) for _ in range(3)]
        grid = td.GridSpec.uniform(dl=DL)
        if rng.integers(0, 2):
            def coords(n, s_):
                d = rng.uniform(0.8, 1.2, n)
                return tuple(np.concatenate(([0.0], np.cumsum(d))) * (s_ / d.sum()) - 0.5 * s_)
            grid = td.GridSpec(grid_x=td.CustomGridBoundaries(coords=coords(N[0], size[0])), grid_y=td.CustomGridBoundaries(coords=coords(N[1], size[1])),
                               grid_z=td.CustomGridBoundaries(coords=coords(N[2], size[2])))
        return td.Simulation(size=size, grid_spec=grid, run_time=1e-12, shutoff=0, subpixel=False, structures=structures,
                             sources=[td.PointDipole(center=pos(), source_time=P3, polarization=str(rng.choice(["Ex", "Ey", "Ez", "Hy"])))],
                             monitors=[td.FieldTimeMonitor(center=pos(), size=(0.2, 0.2, 0.2), name="t", interval=3, colocate=False),
                                       td.FieldMonitor(center=pos(), size=(td.inf, td.inf, 0), freqs=[3e14], name="f")],
                             boundary_spec=td.BoundarySpec(x=edges[0], y=edges[1], z=edges[2]))
    for seed in range(4):
        line(f"test_fully_anisotropic.random_bodies.{seed}", lambda: random_bodies(seed))


def aniso_bloch():
    import test_aniso_bloch as t
    for z in ("bloch", "pml"):
        line(f"test_aniso_bloch.clear_case.{z}", lambda: t.clear_case(z))          # (a Bloch pair: both handles' uploads in the stream)
    sx, sy = 9, 7
    for k, center in enumerate(((0.0, 0.0, 0.0), (sx * t.DL, sy * t.DL, 0.0))):
        line(f"test_aniso_bloch.wrapped_cell.{k}", lambda: t.wrapped_cell(center=center))
    line("test_aniso_bloch.clear_case.small.force_comm", lambda: t.clear_case("bloch", N=(12, 10, 8)), force_comm=True)


def medium2d():
    import test_medium2d as t
    PULSE = t.PULSE
    sheet = td.Medium2D(ss=td.Medium(permittivity=1.0, conductivity=2e-3), tt=td.Drude(eps_inf=1.0, coeffs=[(3e14, 2e13)]))
    zb = np.concatenate([np.linspace(-1.0, 0.0, 21), 0.0 + np.cumsum(np.linspace(0.03, 0.07, 24))])
    zb = zb[zb <= 1.0 + 1e-9]
    grid = td.GridSpec(grid_x=td.UniformGrid(dl=0.05), grid_y=td.UniformGrid(dl=0.05), grid_z=td.CustomGridBoundaries(coords=tuple(zb)))
    for z_sheet, z_glass_top in ((0.0, 0.0), (0.012, 0.0), (0.013, 0.013)):
        line(f"test_medium2d.sheet_nodes.{z_sheet}.{z_glass_top}", lambda: t._sim(sheet, grid=grid, z_sheet=z_sheet, z_glass_top=z_glass_top))
    freqs = np.linspace(1.6e14, 2.4e14, 7)
    mon = [td.FluxMonitor(center=(0, 0, 1.5), size=(td.inf, td.inf, 0), freqs=list(freqs), name="T")]
    line("test_medium2d.plane_wave.empty", lambda: t._plane_wave_sim([], mon))
    for kind, comp in (("conductive", td.Medium(permittivity=1.0, conductivity=2e-3)), ("drude", td.Drude(eps_inf=1.0, coeffs=[(1.2e14, 1.5e13)]))):
        st = td.Structure(geometry=td.Box(center=(0, 0, 0.0), size=(td.inf, td.inf, 0)), medium=td.Medium2D(ss=comp, tt=comp))
        line(f"test_medium2d.plane_wave.{kind}", lambda: t._plane_wave_sim([st], mon))
    r = td.LumpedResistor(center=(0, 0, 0), size=(0.4, 0.2, 0), resistance=75.0, voltage_axis=0, name="R1")
    sim = td.Simulation(size=(1.0, 1.0, 1.0), grid_spec=td.GridSpec.uniform(dl=0.05), run_time=1e-13, subpixel=False,
                        sources=[td.PointDipole(center=(0, 0, 0.3), source_time=PULSE, polarization="Ex")],
                        lumped_elements=[r], boundary_spec=td.BoundarySpec.all_sides(td.PECBoundary()))
    line("test_medium2d.lumped_resistor", lambda: sim)
    cx = td.CoaxialLumpedResistor(center=(0, 0, 0), outer_diameter=0.6, inner_diameter=0.2, normal_axis=2, resistance=50.0, name="C")
    line("test_medium2d.coaxial_resistor", lambda: sim.copy(lumped_elements=(cx,)))


def custom_datasets():
    import test_custom_datasets as t
    PULSE, _const = t.PULSE, t._const
    pec = td.BoundarySpec.all_sides(td.PECBoundary())
    dip = [td.PointDipole(source_time=PULSE, polarization="Ez")]
    x = np.linspace(-0.5, 0.5, 11)
    eps = 2.0 + 2.0 * (x[:, None, None] + 0.5) * np.ones((1, 3, 3))
    sig = 0.01 * np.ones((11, 3, 3))
    sig[:5] = 0.0
    med = td.CustomMedium(permittivity=_spatial(eps, x, [-1, 0, 1], [-1, 0, 1]), conductivity=_spatial(sig, x, [-1, 0, 1], [-1, 0, 1]), interp_method="linear")
    line("test_custom_datasets.raster_interpolation", lambda: td.Simulation(
        size=(2, 1, 1), grid_spec=td.GridSpec.uniform(dl=0.05), run_time=1e-14, subpixel=False,
        structures=[td.Structure(geometry=td.Box(size=(0.8, 0.6, 0.6)), medium=med)], sources=dip, boundary_spec=pec))
    rng = np.random.default_rng(0)
    n = 24
    xx = np.linspace(-0.6, 0.6, n)
    many = td.CustomMedium(permittivity=_spatial(2.0 * 4.0 ** rng.random((n, n, n)), xx, xx, xx),
                           conductivity=_spatial(10.0 ** rng.uniform(-3, -2, (n, n, n)), xx, xx, xx), interp_method="nearest")
    line("test_custom_datasets.many_pairs", lambda: td.Simulation(
        size=(1.2, 1.2, 1.2), grid_spec=td.GridSpec.uniform(dl=0.025), run_time=1e-14, subpixel=False,
        structures=[td.Structure(geometry=td.Box(size=(1.0, 1.0, 1.0)), medium=many)], sources=dip, boundary_spec=pec))

    def slab(medium):
        return td.Simulation(size=(0, 0, 3.0), grid_spec=td.GridSpec.uniform(dl=0.02), run_time=4e-13, shutoff=0,
                             structures=[td.Structure(geometry=td.Box(center=(0, 0, 0.5), size=(td.inf, td.inf, 0.4)), medium=medium)],
                             sources=[td.UniformCurrentSource(center=(0, 0, -1.2), size=(td.inf, td.inf, 0), source_time=PULSE, polarization="Ex")],
                             monitors=[td.FluxMonitor(center=(0, 0, 1.2), size=(td.inf, td.inf, 0), freqs=[1.8e14, 2e14, 2.2e14], name="T")],
                             boundary_spec=td.BoundarySpec(x=td.Boundary.periodic(), y=td.Boundary.periodic(), z=td.Boundary.pml()))
    line("test_custom_datasets.slab.custom", lambda: slab(td.CustomMedium(permittivity=_spatial(np.full((2, 2, 2), 6.25), [-9, 9], [-9, 9], [-9, 9]))))
    line("test_custom_datasets.slab.uniform", lambda: slab(td.Medium(permittivity=6.25)))
    line("test_custom_datasets.slab.custom_drude", lambda: slab(td.CustomDrude(eps_inf=_const(1.0), coeffs=[(_const(3e14), _const(3e13))])))
    line("test_custom_datasets.slab.drude", lambda: slab(td.Drude(eps_inf=1.0, coeffs=[(3e14, 3e13)])))
    # test_triangle_mesh_equals_the_solid_it_bounds
    v = np.array([[x_, y_, z_] for x_ in (-.5, .5) for y_ in (-.3, .3) for z_ in (-.2, .4)])
    faces = [[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]]
    kw = dict(size=(2, 1.6, 1.6), grid_spec=td.GridSpec.uniform(dl=0.05), run_time=1e-14, subpixel=False, sources=dip, boundary_spec=pec)
    m4 = td.Medium(permittivity=4)
    line("test_custom_datasets.mesh.box", lambda: td.Simulation(
        structures=[td.Structure(geometry=td.Box(center=(0.011, 0.007, 0.113), size=(1, 0.6, 0.6)), medium=m4)], **kw))
    line("test_custom_datasets.mesh.mesh", lambda: td.Simulation(
        structures=[td.Structure(geometry=td.TriangleMesh.from_vertices_faces(v + np.array([0.011, 0.007, 0.013]), faces), medium=m4)], **kw))
    # the custom dispersive media
    for name, custom, uniform in t.CUSTOM_DISPERSIVE:
        for what, m in (("custom", custom()), ("uniform", uniform)):
            line(f"test_custom_datasets.dispersive.{name}.{what}", lambda: td.Simulation(
                size=(1, 1, 1), grid_spec=td.GridSpec.uniform(dl=0.05), run_time=1e-14, subpixel=False,
                structures=[td.Structure(geometry=td.Box(size=(0.5, 0.4, 0.6)), medium=m)], sources=dip, boundary_spec=pec))
    xg = np.array([-0.3, -0.1, 0.1, 0.3])
    de = np.array([1.0, 1.0, 2.0, 2.0])[:, None, None] * np.ones((1, 2, 2))
    grp = td.CustomLorentz(eps_inf=_spatial(np.full((4, 2, 2), 2.0), xg, [-9, 9], [-9, 9]),
                           coeffs=[(_spatial(de, xg, [-9, 9], [-9, 9]), _spatial(np.full((4, 2, 2), 3.2e14), xg, [-9, 9], [-9, 9]),
                                    _spatial(np.full((4, 2, 2), 2e13), xg, [-9, 9], [-9, 9]))], interp_method="nearest")
    for what, m in (("nearest", grp), ("linear", td.CustomLorentz(eps_inf=grp.eps_inf, coeffs=grp.coeffs, interp_method="linear"))):
        line(f"test_custom_datasets.groups.{what}", lambda: td.Simulation(
            size=(1, 1, 1), grid_spec=td.GridSpec.uniform(dl=0.05), run_time=1e-14, subpixel=False,
            structures=[td.Structure(geometry=td.Box(size=(0.8, 0.4, 0.6)), medium=m)], sources=dip, boundary_spec=pec))
    # test_autogrid_sizes_its_steps_with_the_largest_permittivity_of_the_data
    xa = np.linspace(-0.5, 0.5, 5)
    ea = np.array([2.0, 2.0, 4.0, 9.0, 2.0])[:, None, None] * np.ones((1, 2, 2))
    for what, m in (("custom", td.CustomMedium(permittivity=_spatial(ea, xa, [-9, 9], [-9, 9]))), ("uniform", td.Medium(permittivity=9.0))):
        line(f"test_custom_datasets.autogrid.{what}", lambda: td.Simulation(
            size=(3, 1, 1), grid_spec=td.GridSpec.auto(min_steps_per_wvl=12, wavelength=1.5), run_time=1e-14,
            structures=[td.Structure(geometry=td.Box(size=(1.0, td.inf, td.inf)), medium=m)],
            sources=[td.PointDipole(center=(1.2, 0, 0), source_time=PULSE, polarization="Ez")], boundary_spec=pec))
    # test_custom_anisotropic_and_perturbation_media
    xc = np.array([-0.3, 0.3])
    exx = np.array([2.0, 4.0])[:, None, None] * np.ones((1, 2, 2))
    ca = td.CustomAnisotropicMedium(xx=td.CustomMedium(permittivity=_spatial(exx, xc, [-9, 9], [-9, 9]), interp_method="nearest"),
                                    yy=td.Medium(permittivity=3.0), zz=td.CustomDrude(eps_inf=_const(1.5), coeffs=[(_const(4e14), _const(3e13))]))
    line("test_custom_datasets.custom_anisotropic", lambda: td.Simulation(
        size=(1, 1, 1), grid_spec=td.GridSpec.uniform(dl=0.05), run_time=1e-14, subpixel=False,
        structures=[td.Structure(geometry=td.Box(size=(0.8, 0.4, 0.6)), medium=ca)], sources=dip, boundary_spec=pec))
    # a fully anisotropic sphere under a custom block (the custom branch takes the tagged nodes over), and a Kerr / a modulated box under one
    import modulation_case
    import nonlinear_case
    blk = td.CustomMedium(permittivity=_spatial(exx, xc, [-9, 9], [-9, 9]), interp_method="nearest")
    fa = td.FullyAnisotropicMedium(permittivity=[[2.5, 0.3, 0.0], [0.3, 2.2, 0.1], [0.0, 0.1, 2.0]])
    for what, m in (("aniso", fa), ("kerr", nonlinear_case.kerr(eps=3.0)), ("modulated", modulation_case.eps_modulated(eps=3.0, amp=0.5))):
        line(f"custom_block_over.{what}", lambda: td.Simulation(
            size=(1, 1, 1), grid_spec=td.GridSpec.uniform(dl=0.05), run_time=1e-14, subpixel=False,
            structures=[td.Structure(geometry=td.Sphere(center=(0.05, 0, 0), radius=0.3), medium=m),
                        td.Structure(geometry=td.Box(center=(0.2, 0.1, 0), size=(0.4, 0.4, 0.3)), medium=blk)], sources=dip, boundary_spec=pec))


def wide_media():
    import test_wide_media as t
    line("test_wide_media.emulator", lambda: t.wide_sim((28, 24, 20), 24, eps_span=2.0, sig_span=10.0))
    line("test_wide_media.one_coarsening_step", lambda: t.wide_sim((28, 24, 20), 24))
    line("test_wide_media.device", lambda: t.wide_sim((96, 80, 64), 48, eps_span=3.0))


# Scenes of the files above that are left out, with the reason (at most one in ten):
LEFT_OUT = [
    ("test_custom_datasets.test_reference_sample_file_loads_with_its_datasets", "needs the reference checkout's sample file; skipped by the suite without it"),
    ("test_custom_datasets.test_reference_sample_file_custom_dispersive_media_carry_their_data", "likewise"),
    ("test_custom_datasets.test_custom_field_and_current_sources_on_the_oracle", "custom source datasets written to a temporary file: no structure, no list"),
]


if __name__ == "__main__":
    cases_and_scenarios()
    fully_anisotropic()
    aniso_bloch()
    medium2d()
    custom_datasets()
    wide_media()
    for name, why in LEFT_OUT:
        print(f"left out: {name} ({why})")
