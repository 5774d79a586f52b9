"""512^3 V2 (bench.py build_spec) with a 300-cell cube FieldMonitor, six fields, five frequencies, interval_space = (4, 4, 4): host
path and device path alternated twice in one process, 10 warm-up + 100 timed steps each; device bytes of the monitor; results() and
assemble times."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import tidy3d_amd.schema as td
from tidy3d_amd.discretize import discretize
from tidy3d_amd.engine import HipEngine
from tidy3d_amd.data import assemble

n, dl, warm, timed = 512, 0.05, 10, 100
size = ((n - 24) * dl - 1e-6 * dl,) * 3
freqs = tuple(np.linspace(1.8e14, 2.2e14, 5))
sim = td.Simulation(size=size, grid_spec=td.GridSpec.uniform(dl=dl), run_time=1e-12,
                    structures=[td.Structure(geometry=td.Sphere(center=(0, 0, 0), radius=100 * dl), medium=td.Medium(permittivity=4.0))],
                    sources=[td.PointDipole(center=(0, 0, 0), source_time=td.GaussianPulse(freq0=2e14, fwidth=2e13), polarization="Ez")],
                    monitors=[td.FieldMonitor(center=(0, 0, 0), size=(300 * dl,) * 3, name="cube", freqs=freqs, interval_space=(4, 4, 4))],
                    boundary_spec=td.BoundarySpec.all_sides(td.PML(num_layers=12)), shutoff=0)
out = open(sys.argv[1] if len(sys.argv) > 1 else os.devnull, "a")          # usage: python profiles/field_dft/dft_512.py [OUT.jsonl]
def say(**kw):
    print(json.dumps(kw), flush=True); out.write(json.dumps(kw) + "\n"); out.flush()
t = time.perf_counter()
discs = {"host": discretize(sim, n_steps=warm + timed, field_dft_device=False), "device": discretize(sim, n_steps=warm + timed, field_dft_device=True)}
for d in discs.values():
    d.spec.decay_every = 0
say(event="discretized", s=time.perf_counter() - t, kinds={k: d.spec.monitors[0].kind for k, d in discs.items()}, nyquist=int(discs["host"].nyquist_step),
    box=discs["host"].spec.monitors[0].shape, n_rec=len(discs["host"].spec.monitors[0].steps), targets=discs["device"].spec.monitors[0].targets[0])
for rnd in (1, 2):
    for path in ("host", "device"):
        disc = discs[path]
        with HipEngine(disc.spec, device=0) as e:
            e.run(warm)
            t = time.perf_counter(); st = e.run(timed); wall = time.perf_counter() - t
            row = dict(event="run", round=rnd, path=path, ms_per_step_wall=1e3 * wall / timed, run_ms_per_step=float(st.run_ms) / timed,
                       fused2_pairs=int(st.fused2_pairs), axis_shift=int(e.axis_shift), bytes=e.monitor_bytes("cube", detail=True))
            say(**row)
            if rnd == 1:
                t = time.perf_counter(); raw = e.results(); row = dict(event="results", path=path, results_s=time.perf_counter() - t, raw_shape=list(raw["cube"].shape))
                say(**row)
                t = time.perf_counter(); sd = assemble(disc, raw)
                say(event="assemble", path=path, assemble_s=time.perf_counter() - t, Ez_shape=list(sd["cube"].Ez.values.shape))
                del raw, sd
