"""Wall time and peak memory of `discretize(sim, n_steps=2)` for 256 x 256 x 192 scenes with a dozen Box, Sphere and Cylinder bodies: what
the rasteriser's tag volumes cost at set-up (docs/history/LIST_SETUP.md).  CPU only.

    python profiles/list_setup/raster_time.py run SCENE LABEL >> log      # one scene, one fresh process: one JSON line
    python profiles/list_setup/raster_time.py check log                    # the runs labelled "here" against those labelled "parent"

Scenes: "plain" (plain media only: no tag volume may be allocated), "kerr" (one Box a Kerr medium), "aniso" (one Sphere a
FullyAnisotropicMedium) — the last two apart, since the two kinds are refused together.  `check`: the runs of this tree lie within the
span of the parent's, widened by that span again on either side; the plain scene's peak RSS does not exceed the parent's largest by a
uint8 volume of the grid."""
import json
import os
import resource
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, ROOT)
N = (256, 256, 192)
DL = 0.05
SCENES = ("plain", "kerr", "aniso")


def scene(name):
    import tidy3d_amd.schema as td
    import numpy as np
    L = [float(np.sum((DL,) * n)) for n in N]          # exactly N cells of DL per axis
    m = [td.Medium(permittivity=2.0 + 0.5 * k) for k in range(4)]
    kerr = td.Medium(permittivity=3.0, nonlinear_spec=td.NonlinearSpec(models=(td.NonlinearSusceptibility(chi3=1e-3),), num_iters=5))
    fa = td.FullyAnisotropicMedium(permittivity=[[2.5, 0.3, 0.0], [0.3, 2.2, 0.1], [0.0, 0.1, 2.0]])
    bodies = [
        (td.Box(center=(0, 0, -0.3 * L[2]), size=(td.inf, td.inf, 0.3 * L[2])), m[0]),                  # a substrate: the threaded slice fill
        (td.Box(center=(-0.2 * L[0], 0.1 * L[1], 0.05 * L[2]), size=(0.3 * L[0], 0.4 * L[1], 0.3 * L[2])), kerr if name == "kerr" else m[1]),
        (td.Sphere(center=(0.2 * L[0], -0.15 * L[1], 0.1 * L[2]), radius=0.15 * L[0]), fa if name == "aniso" else m[2]),
        (td.Cylinder(center=(0.1 * L[0], 0.25 * L[1], 0), radius=0.08 * L[0], length=0.5 * L[2], axis=2), m[3]),
        (td.Box(center=(0.3 * L[0], 0.3 * L[1], 0.2 * L[2]), size=(0.2 * L[0], 0.2 * L[1], 0.2 * L[2])), m[0]),
        (td.Sphere(center=(-0.3 * L[0], -0.3 * L[1], 0.25 * L[2]), radius=0.1 * L[0]), m[1]),
        (td.Cylinder(center=(-0.1 * L[0], -0.2 * L[1], 0.1 * L[2]), radius=0.06 * L[0], length=0.6 * L[1], axis=1), m[2]),
        (td.Box(center=(-0.25 * L[0], 0.12 * L[1], 0.08 * L[2]), size=(0.1 * L[0], 0.2 * L[1], 0.1 * L[2])), m[3]),      # into the second body
        (td.Sphere(center=(0.25 * L[0], -0.1 * L[1], 0.15 * L[2]), radius=0.07 * L[0]), m[0]),                         # into the third
        (td.Box(center=(0, 0, 0.4 * L[2]), size=(td.inf, 0.1 * L[1], 0.05 * L[2])), m[1]),
        (td.Cylinder(center=(0.35 * L[0], 0, -0.05 * L[2]), radius=0.05 * L[0], length=0.3 * L[0], axis=0), m[2]),
        (td.Sphere(center=(0, 0.35 * L[1], 0.3 * L[2]), radius=0.08 * L[0]), m[3]),
    ]
    pec = td.Boundary(minus=td.PECBoundary(), plus=td.PECBoundary())
    return td.Simulation(size=tuple(L), grid_spec=td.GridSpec(grid_x=td.CustomGrid(dl=(DL,) * N[0]), grid_y=td.CustomGrid(dl=(DL,) * N[1]),
                                                                  grid_z=td.CustomGrid(dl=(DL,) * N[2])), run_time=1e-13, subpixel=False, shutoff=0,
                         structures=[td.Structure(geometry=g, medium=med) for g, med in bodies],
                         sources=[td.PointDipole(center=(0, 0, 0), source_time=td.GaussianPulse(freq0=3e14, fwidth=1.5e14), polarization="Ez")],
                         boundary_spec=td.BoundarySpec(x=pec, y=pec, z=pec))


def run(name, label):
    from tidy3d_amd.discretize import discretize
    sim = scene(name)
    t0 = time.perf_counter()
    spec = discretize(sim, n_steps=2).spec
    seconds = time.perf_counter() - t0
    assert spec.shape == N, spec.shape
    if name == "plain":
        assert spec.aniso == [] and not spec.modulation and not spec.nonlinear
    else:
        assert (spec.nonlinear if name == "kerr" else spec.aniso)
    print(json.dumps({"tree": label, "scene": name, "seconds": round(seconds, 3), "peak_rss_kb": resource.getrusage(resource.RUSAGE_SELF).ru_maxrss,
                      "listed_nodes": sum(len(s.ijk) for s in spec.nonlinear + spec.aniso)}), flush=True)


def check(path):
    rows = [json.loads(ln) for ln in open(path) if ln.startswith("{")]
    ok = True
    for name in SCENES:
        t = {lab: [r["seconds"] for r in rows if r["scene"] == name and r["tree"] == lab] for lab in ("parent", "here")}
        span = max(t["parent"]) - min(t["parent"])
        lo, hi = min(t["parent"]) - span, max(t["parent"]) + span
        inside = all(lo <= v <= hi for v in t["here"])
        print(f"{name}: parent {t['parent']} s, here {t['here']} s, allowed [{lo:.3f}, {hi:.3f}]: {'inside' if inside else 'OUTSIDE'}")
        ok &= inside or max(t["here"]) <= hi           # (faster than the parent is no failure)
    rss = {lab: max(r["peak_rss_kb"] for r in rows if r["scene"] == "plain" and r["tree"] == lab) for lab in ("parent", "here")}
    volume_kb = 3 * N[0] * N[1] * N[2] // 1024
    print(f"plain: peak RSS parent {rss['parent']} kB, here {rss['here']} kB, one uint8 volume {volume_kb} kB")
    assert rss["here"] < rss["parent"] + volume_kb, "a tag volume was allocated for plain media"
    assert ok, "set-up is slower than the parent's span allows"


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(sys.argv[2], sys.argv[3])
    else:
        check(sys.argv[2])
