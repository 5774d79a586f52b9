"""320^3 vacuum, PEC walls, a slab of 320 x 320 x 40 cells — a plain dielectric or the same dielectric modulated in time (~12 M listed
nodes over the three components) — on single steps (FDTD_OPT_TWOSTEP = 0): ms per step of 100 steps, three repeats, one JSON line.
    python profiles/modulation/slab_320.py plain|modulated        (run from the root of the tree whose package is to be measured)"""
import json
import os
import sys

sys.path.insert(0, os.getcwd())
import numpy as np

import tidy3d_amd.schema as td
from tidy3d_amd import lib as L
from tidy3d_amd.discretize import discretize
from tidy3d_amd.engine import HipEngine

kind = sys.argv[1]
N, DL, STEPS = 320, 0.05, 100
if kind == "modulated":
    stm = td.SpaceTimeModulation(time_modulation=td.ContinuousWaveTimeModulation(freq0=1e14, amplitude=0.5))
    med = td.Medium(permittivity=2.25, modulation_spec=td.ModulationSpec(permittivity=stm))
else:
    med = td.Medium(permittivity=2.25)
wall = td.Boundary(minus=td.PECBoundary(), plus=td.PECBoundary())
grid = td.GridSpec(grid_x=td.CustomGrid(dl=(DL,) * N), grid_y=td.CustomGrid(dl=(DL,) * N), grid_z=td.CustomGrid(dl=(DL,) * N))
sim = td.Simulation(size=(float(np.sum((DL,) * N)),) * 3, grid_spec=grid, run_time=1e-12, subpixel=False,
                    structures=[td.Structure(geometry=td.Box(center=(0, 0, 0), size=(td.inf, td.inf, 40 * DL)), medium=med)],
                    sources=[td.PointDipole(center=(0.3, 0.2, 4.0), source_time=td.GaussianPulse(freq0=3e14, fwidth=1.5e14), polarization="Ez")],
                    monitors=[], boundary_spec=td.BoundarySpec(x=wall, y=wall, z=wall), shutoff=0)
spec = discretize(sim, n_steps=10 + 3 * STEPS).spec
spec.decay_every = 0
listed = sum(len(m.ijk) for m in getattr(spec, "modulation", []))
with HipEngine(spec, lib=L.load_library()) as e:
    e.set_option(L.OPT_TWOSTEP, 0)
    e.run(10)
    ms = []
    for _ in range(3):
        st = e.run(STEPS)
        ms.append(float(st.run_ms) / STEPS)
    assert int(st.fused2_pairs) == 0
    amp = float(np.abs(e.get_field(2)).max())
print(json.dumps({"tree": os.path.basename(os.getcwd()), "slab": kind, "shape": list(spec.shape), "listed_nodes": listed,
                  "ms_per_step": [round(v, 4) for v in ms], "off_reason": int(st.fused2_off_reason), "max_abs_ez": amp}))
