"""Directivity of a short z dipole in vacuum: a `DirectivityMonitor` box around a `PointDipole`, the flux through the box reduced on
the device from the lattice accumulators (`projection_device=True`).  Prints the peak directivity beside the formula's 1.5 (the
pattern is 1.5 sin^2(theta)), the radiated power and the axial ratio in the equatorial plane (linear: the cap of 100).

    python examples/dipole_directivity.py        # needs an MI355X and the built library
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))      # run from a checkout
import tidy3d_amd
import tidy3d_amd.schema as td

f0 = 3e14                                            # 1 um
dl = 1 / 30
theta = np.linspace(0, np.pi, 37)
phi = np.linspace(0, 2 * np.pi, 12, endpoint=False)
sim = td.Simulation(size=(2.4, 2.4, 2.4), grid_spec=td.GridSpec.uniform(dl=dl), run_time=8e-14,
                    sources=[td.PointDipole(center=(0, 0, 0), source_time=td.GaussianPulse(freq0=f0, fwidth=f0 / 5), polarization="Ez")],
                    monitors=[td.DirectivityMonitor(center=(0, 0, 0), size=(1.6, 1.6, 1.6), freqs=[f0], theta=theta, phi=phi, name="antenna")],
                    boundary_spec=td.BoundarySpec.all_sides(td.PML(num_layers=12)), shutoff=1e-5)
data = tidy3d_amd.run(sim, task_name="dipole_directivity", verbose=False, projection_device=True)
for line in data.log.splitlines():
    if "Flux of DirectivityMonitor" in line or "Time-stepping speed" in line:
        print("   ", line)
d = data["antenna"]
D = np.asarray(d.directivity.values)[0, :, :, 0]
i, j = np.unravel_index(np.argmax(D), D.shape)
print(f"peak directivity {D.max():.4f} at theta = {np.degrees(theta[i]):.1f} deg (formula: 1.5 at 90 deg)")
print(f"largest deviation from 1.5 sin^2(theta): {np.abs(D - 1.5 * np.sin(theta)[:, None] ** 2).max():.4f}")
print(f"radiated power {float(d.flux.values[0]):.5g} W; axial ratio at theta = 90 deg: {float(d.axial_ratio.values[0, 18, 0, 0]):.1f} (linear: capped at 100)")
assert abs(D.max() - 1.5) < 0.05
