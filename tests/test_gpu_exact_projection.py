"""Exact projection (far_field_approx=False) with its surface integrals on the MI355X: ``fdtd_near_field`` (kernel K9b,
csrc/fdtd_near_field.hpp) against the longdouble reference of tests/exact_projection_case.py, held to 8 x the floor the host
path's float64 arithmetic leaves against it — the cases and the checks of tests/test_emu_exact_projection.py through the product
library, and one mid-size call.  Device against emulator: both are held to the same reference by the same bar on the same cases
(the emulator in tests/test_emu_exact_projection.py; building the emulated library is no work for a GPU test) — not to equal bits:
the host compiler's and the device compiler's math libraries and contractions differ."""
import numpy as np
import pytest

from tidy3d_amd import web
from tidy3d_amd.data import assemble
from tidy3d_amd.discretize import discretize

import exact_projection_case as xc
from flux_time_case import run_engine

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(xc.CASES))
def test_twelve_sums_within_eight_floors(hip_lib, name):
    got = xc.check_case(hip_lib, name, "device")
    again = xc.device_sums(hip_lib, name)
    assert np.array_equal(got.view(np.float64), again.view(np.float64)), name          # two calls: equal bits
    if name in xc.CHUNKS:
        assert hip_lib.near_field_chunks(*(xc.CASES[name][i] for i in (2, 0, 1))) == xc.CHUNKS[name]


def test_no_points_and_bad_arguments(hip_lib):
    from test_emu_exact_projection import test_no_points_and_bad_arguments as check
    check(hip_lib)


def test_mid_size_call(hip_lib):
    name = xc.MID_SIZE[0]
    got = xc.check_case(hip_lib, name, "device")
    assert hip_lib.near_field_chunks(64 * 64, 96, 96) == 1
    assert np.isfinite(got).all()
    again = xc.device_sums(hip_lib, name)
    assert np.array_equal(got.view(np.float64), again.view(np.float64))


def test_end_to_end(hip_lib):
    disc = discretize(xc.simulation(), n_steps=xc.N_STEPS)
    raw, _ = run_engine(disc.spec, hip_lib)
    dev, host = (assemble(disc, raw, device_lib=hip_lib, exact_projection_device=mode) for mode in (True, False))
    xc.same_containers(dev, host)
    ref = xc.end_to_end_reference(disc, raw)
    floor, f_at = xc.end_deviation(host, ref)
    d, at = xc.end_deviation(dev, ref)
    print(f"[exact projection] device end to end: floor {floor:.3e} {f_at}, deviation {d:.3e} {at}, ratio {d / floor:.3f} (bar {xc.FACTOR})")
    assert floor > 0 and d <= xc.FACTOR * floor, (d, floor, at)
    assert {n: p for n, (p, _) in xc.log_paths(dev).items()} == {"box": "device", "lossy": "device"}
    sd = web.run(xc.simulation(), n_steps=xc.N_STEPS, verbose=False, exact_projection_device=True)
    assert {n: p for n, (p, _) in xc.log_paths(sd).items()} == {"box": "device", "lossy": "device"}
    xc.same_values(sd, dev)
    auto = web.run(xc.simulation(), n_steps=xc.N_STEPS, verbose=False)
    assert {n: p for n, (p, _) in xc.log_paths(auto).items()} == {"box": "host", "lossy": "host"}
    xc.same_values(auto, host)
