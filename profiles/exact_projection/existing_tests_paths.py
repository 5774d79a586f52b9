#!/usr/bin/env python
"""Which path the exact projections of the EXISTING tests take under the default selection (exact_projection_device=None): the log
line of data.assemble for tests/projection_dft_case.py (`cart`, through web.run with the emulated library) and the pair counts of
the monitors of tests/test_projection.py (assembled without a library: host whatever the count)."""
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "hipemu")]

import build_emu                                    # noqa: E402
import tidy3d_amd.schema as td                      # noqa: E402
from tidy3d_amd import projection, web              # noqa: E402
from tidy3d_amd.discretize import discretize        # noqa: E402
from tidy3d_amd.lib import load_library             # noqa: E402
import projection_dft_case as pc                    # noqa: E402

lib = load_library(build_emu.build())
for dev in (True, False):
    sd = web.run(pc.simulation(), lib=lib, n_steps=pc.N_STEPS, verbose=False, projection_device=dev)
    print(f"projection_dft_case, projection_device={dev}:", [ln for ln in sd.log.split("\n") if ln.startswith("Exact projection")])
f0 = 3e14
pulse = td.GaussianPulse(freq0=f0, fwidth=f0 / 6)
box = dict(center=(0, 0, 0), size=(1.0, 1.0, 1.0), freqs=[f0], far_field_approx=False)
sim = td.Simulation(size=(2.2, 2.2, 2.2), grid_spec=td.GridSpec.uniform(dl=1 / 20), run_time=30 / f0,
                    sources=[td.PointDipole(center=(0, 0, 0), source_time=pulse, polarization="Ex")],
                    monitors=[td.FieldProjectionCartesianMonitor(x=[0.3, 0.45], y=[0.2], proj_distance=0.8, proj_axis=2, name="near", **box),
                              td.FieldProjectionAngleMonitor(theta=[0.7, 1.9], phi=[0.4], proj_distance=3e3, name="exact", **box)],
                    boundary_spec=td.BoundarySpec.all_sides(td.PML(num_layers=8)), shutoff=1e-5)
disc = discretize(sim)
for plan in disc.plans:
    print(f"test_projection.py '{plan.monitor.name}': {projection.exact_pairs(disc, plan, 2)} pairs (threshold {projection.EXACT_HOST_PAIRS})")
