#!/usr/bin/env python
"""320^3, CPML on all faces, a CustomMedium block over about half the volume that runs into the x layers, ~5000 table entries:
the two-pass kernels (VARIANT_ZMARCH, what a wide table ran before), the wide fused sweep, and the same data quantised coarsely
enough for the narrow table on fused single steps (the ceiling).  Three engines in ONE process, alternated twice, 10 warm-up +
100 timed steps each (placement noise between processes is 3-5 %).  One JSON line per timed run.

    python profiles/wide_sweep/wide_320.py [N] [out.jsonl]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(0, ROOT)

import tidy3d_amd.schema as td                        # noqa: E402
from tidy3d_amd import lib as L                       # noqa: E402
from tidy3d_amd.data import DataArray                 # noqa: E402
from tidy3d_amd.discretize import discretize          # noqa: E402
from tidy3d_amd.engine import HipEngine               # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 320
OUT = sys.argv[2] if len(sys.argv) > 2 else None
DL = 0.05
LAYERS = 12                # the layers are added outside `size`: N counts them
WARM, STEPS = 10, 100


def spatial(values, axes):
    a = DataArray(np.asarray(values), {k: np.asarray(v, float) for k, v in zip("xyz", axes)})
    a.tag = "SpatialDataArray"
    return a


def sim(coarse):
    rng = np.random.default_rng(0)
    size = ((N - 2 * LAYERS) * DL,) * 3
    n_data = 48
    ax = [np.linspace(-0.5 * s, 0.5 * s, n_data) for s in size]
    eps = 2.0 * 3.0 ** rng.random((n_data,) * 3)
    sig = 0.01 * 3.0 ** rng.random((n_data,) * 3)
    if coarse:      # 3 % steps in permittivity, 20 % in conductivity: a few hundred pairs
        eps = np.exp(np.round(np.log(eps) / 0.03) * 0.03)
        sig = np.exp(np.round(np.log(sig) / 0.2) * 0.2)
    med = td.CustomMedium(permittivity=spatial(eps, ax), conductivity=spatial(sig, ax), interp_method="nearest")
    pulse = td.GaussianPulse(freq0=3e14, fwidth=1.5e14)
    return td.Simulation(
        size=size, grid_spec=td.GridSpec.uniform(dl=DL), run_time=1e-12, subpixel=False, shutoff=0,
        structures=[td.Structure(geometry=td.Box(center=(0, 0.1 * size[1], 0), size=(td.inf, 0.7 * size[1], 0.7 * size[2])), medium=med)],
        sources=[td.PointDipole(center=(0.02, 0.01, 0.03), source_time=pulse, polarization="Ez")],
        monitors=[td.FieldTimeMonitor(center=(0.1, 0.1, 0.05), size=(0, 0, 0), name="probe", interval=10, colocate=False)],
        boundary_spec=td.BoundarySpec.all_sides(td.PML(num_layers=LAYERS)))


def main():
    t0 = time.time()
    wide = discretize(sim(False), n_steps=WARM + STEPS).spec
    narrow = discretize(sim(True), n_steps=WARM + STEPS).spec
    print(f"grid {wide.shape}: {len(wide.media)} media in the wide table, {len(narrow.media)} in the narrow one "
          f"(discretised in {time.time() - t0:.0f} s)", flush=True)
    assert len(wide.media) > 1023 >= len(narrow.media)
    cells = float(np.prod(wide.shape))
    runs = [("zmarch_wide", wide, L.VARIANT_ZMARCH, {}),
            ("fused_wide", wide, L.VARIANT_FUSED, {}),
            ("fused_narrow_single_steps", narrow, L.VARIANT_FUSED, {L.OPT_TWOSTEP: 0, L.OPT_SHELL_PAIRS: 0})]
    engines = []
    for name, spec, variant, opts in runs:
        e = HipEngine(spec, variant=variant)
        for k, v in opts.items():
            e.set_option(k, v)
        engines.append((name, e))
    lines = []
    for rep in range(2):
        for name, e in engines:
            e.reset()
            e.run(WARM)
            st = e.run(STEPS)
            ms = float(st.run_ms) / STEPS
            rec = {"run": name, "repeat": rep, "ms_per_step": round(ms, 4), "gcells_per_s": round(cells / ms * 1e-6, 1),
                   "media": len(e.spec.media), "fused2_pairs": int(st.fused2_pairs), "off_reason": int(st.fused2_off_reason),
                   "diverged": int(st.diverged)}
            print(json.dumps(rec), flush=True)
            lines.append(rec)
    for _, e in engines:
        e.close()
    if OUT:
        os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
        with open(OUT, "w") as f:
            f.write(json.dumps({"grid": list(wide.shape), "media_wide": len(wide.media), "media_narrow": len(narrow.media)}) + "\n")
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
