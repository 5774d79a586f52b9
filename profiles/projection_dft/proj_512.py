"""512^3 V2 (bench.py build_spec sizes) with a sphere, a dipole and a closed FieldProjectionAngleMonitor box of 440 cells a side, 25
frequencies: host path (whole-box accumulators) and device path (lattice accumulators, projection_device=True) alternated twice in
one process, 10 warm-up + 100 timed steps each; device bytes of the monitor; results() time and the host seconds
projection._surface_currents takes on either path."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import tidy3d_amd.schema as td
from tidy3d_amd import projection
from tidy3d_amd.data import source_spectrum_fn
from tidy3d_amd.discretize import discretize
from tidy3d_amd.engine import HipEngine

n, dl, warm, timed = 512, 0.05, 10, 100
size = ((n - 24) * dl - 1e-6 * dl,) * 3
freqs = tuple(np.linspace(1.8e14, 2.2e14, 25))
sim = td.Simulation(size=size, grid_spec=td.GridSpec.uniform(dl=dl), run_time=1e-12,
                    structures=[td.Structure(geometry=td.Sphere(center=(0, 0, 0), radius=100 * dl), medium=td.Medium(permittivity=4.0))],
                    sources=[td.PointDipole(center=(0, 0, 0), source_time=td.GaussianPulse(freq0=2e14, fwidth=2e13), polarization="Ez")],
                    monitors=[td.FieldProjectionAngleMonitor(center=(0, 0, 0), size=(440 * dl,) * 3, name="far", freqs=freqs, theta=(0.5, 1.5), phi=(0.0, 1.0))],
                    boundary_spec=td.BoundarySpec.all_sides(td.PML(num_layers=12)), shutoff=0)
out = open(sys.argv[1] if len(sys.argv) > 1 else os.devnull, "a")          # usage: python profiles/projection_dft/proj_512.py [OUT.jsonl]
def say(**kw):
    print(json.dumps(kw), flush=True); out.write(json.dumps(kw) + "\n"); out.flush()
t = time.perf_counter()
discs = {"host": discretize(sim, n_steps=warm + timed, projection_device=False), "device": discretize(sim, n_steps=warm + timed, projection_device=True)}
auto = discretize(sim, n_steps=warm + timed)
for d in discs.values():
    d.spec.decay_every = 0
say(event="discretized", s=time.perf_counter() - t, kinds={k: sorted({m.kind for m in d.spec.monitors}) for k, d in discs.items()},
    kinds_none=sorted({m.kind for m in auto.spec.monitors}), nyquist=int(discs["host"].nyquist_step), n_rec=len(discs["host"].spec.monitors[0].steps),
    boxes=[list(m.shape) for m in discs["host"].spec.monitors], lattices=[list(m.targets[0]) for m in discs["device"].spec.monitors])
for rnd in (1, 2):
    for path in ("host", "device"):
        disc = discs[path]
        with HipEngine(disc.spec, device=0) as e:
            e.run(warm)
            t = time.perf_counter(); st = e.run(timed); wall = time.perf_counter() - t
            say(event="run", round=rnd, path=path, ms_per_step_wall=1e3 * wall / timed, run_ms_per_step=float(st.run_ms) / timed,
                fused2_pairs=int(st.fused2_pairs), axis_shift=int(e.axis_shift), bytes=e.monitor_bytes("far", detail=True))
            if rnd == 1:
                t = time.perf_counter(); raw = e.results()
                say(event="results", path=path, results_s=time.perf_counter() - t, raw_bytes=int(sum(v.nbytes for v in raw.values())))
                plan, norm = disc.plans[0], source_spectrum_fn(disc, disc.sim.normalize_index)
                t = time.perf_counter()
                n_surf = sum(1 for _ in projection._surface_currents(disc, plan, raw, norm, sim.medium))
                say(event="surface_currents", path=path, surface_currents_s=time.perf_counter() - t, surfaces=n_surf)
                del raw
