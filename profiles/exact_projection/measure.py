#!/usr/bin/env python
"""Exact projection, one surface, one frequency: a 256 x 256 lattice and 128 x 128 observation points (1.07e9 point-node pairs).

    python profiles/exact_projection/measure.py [--device-only]

Device: whole-call wall time of ``lib.near_field`` (allocate, upload, two kernels, download, free), three repeats after one warm-up.
Host: the NumPy statements of ``projection._exact_fields`` (``exact_projection_case.twelve_sums`` in float64) on 64 of the points,
SCALED by the point count.  Prints one JSON line.  Kernel time: run this under ``rocprofv3 --kernel-trace --stats`` with --device-only."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from tidy3d_amd.lib import load_library          # noqa: E402
from tidy3d_amd.projection import _trap_weights  # noqa: E402
import exact_projection_case as xc               # noqa: E402

rng = np.random.default_rng(5)
u = v = (np.arange(256) - 127.5) * 0.1
cur = rng.standard_normal((4, 256, 256)) + 1j * rng.standard_normal((4, 256, 256))
g = np.linspace(-8.0, 8.0, 128)
pu, pv = (a.ravel() for a in np.meshgrid(g, g + 0.013, indexing="ij"))
pw = np.full(pu.size, 20.25)
k = 2 * np.pi * (1 + 0.002j)
w = _trap_weights(u)
lib = load_library()
res = {"lattice": [256, 256], "points": int(pu.size), "pairs": int(pu.size) * 256 * 256, "chunks": lib.near_field_chunks(pu.size, 256, 256)}
call = lambda: lib.near_field(u, v, w, w, cur, 0.25, k, pu, pv, pw)      # noqa: E731
got = call()
times = []
for _ in range(3):
    t = time.perf_counter()
    again = call()
    times.append(time.perf_counter() - t)
res["device_call_s"] = times
res["equal_bits"] = bool(np.array_equal(got.view(np.float64), again.view(np.float64)))
if "--device-only" not in sys.argv:
    idx = np.linspace(0, pu.size - 1, 64).round().astype(int)
    t = time.perf_counter()
    host = xc.twelve_sums(u, v, 0.25, cur, k, pu[idx], pv[idx], pw[idx])
    dt = time.perf_counter() - t
    res["host_64_points_s"] = dt
    res["host_scaled_s"] = dt * pu.size / 64
    res["host_scaled_over_device"] = res["host_scaled_s"] / float(np.median(times))
    res["device_vs_host_on_64_points"] = xc.deviation(got[idx], host.astype(np.clongdouble))[0]
print(json.dumps(res))
