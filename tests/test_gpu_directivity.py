"""The flux of a DirectivityMonitor reduced on the device (``lattice_flux_kernel``, csrc/fdtd_lattice_flux.hpp) on the product
library: the checks of tests/test_emu_directivity.py — every scene with the split run and the repeat after fdtd_reset — and
web.run of scene A with the flux on the device against the host path."""
import numpy as np
import pytest

import directivity_case as case
import test_emu_directivity as emu

pytestmark = pytest.mark.gpu


def test_the_entry_points_are_there(hip_lib):
    emu.test_the_entry_points_are_there(hip_lib)


def test_kernel_scene_a(hip_lib):
    emu.check_kernel_a(hip_lib, repeat=True)


@pytest.mark.parametrize("scene", ["b", "c"])
def test_kernel_scenes_b_and_c(hip_lib, scene):
    emu.test_kernel_scenes_b_and_c(hip_lib, scene)


def test_renamed_axes(hip_lib):
    for shift in (1, 2):
        emu.test_renamed_axes(hip_lib, shift)


def test_device_against_host_end_to_end(hip_lib):
    """scene A through web.run: projection_device=True against False"""
    runs = [case.run_scene_a(hip_lib, dev) for dev in (True, False)]
    emu.end_to_end(hip_lib, None, None, runs=runs)
    d = runs[0]["dir"]
    assert type(d).__name__ == "DirectivityData" and np.asarray(d.directivity.values).shape == (1, 13, 8, 2)
    assert np.isfinite(np.asarray(d.directivity.values)).all()
    for c in ("Etheta", "Ephi", "Htheta", "Hphi"):             # ... and on the device path too the far fields are the angle monitor's
        assert np.array_equal(np.asarray(getattr(d, c).values), np.asarray(getattr(runs[0]["ang"], c).values)), c


def test_web_run_tiny_scene_and_refusals(hip_lib):
    emu.test_web_run_on_both_paths(hip_lib)
    emu.library_refusals(hip_lib)
