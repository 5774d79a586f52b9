"""Box, Sphere and Cylinder structures rasterised on the device (``raster_paint_kernel``, csrc/fdtd_raster.hpp) on the product
library: the checks of tests/test_emu_raster.py — every scene against the host path's arrays, bit for bit."""
import pytest

import test_emu_raster as emu

pytestmark = pytest.mark.gpu


def test_the_entry_point_is_there(hip_lib):
    emu.test_the_entry_point_is_there(hip_lib)


def test_boxes_and_snapped_faces(hip_lib):
    emu.boxes(hip_lib)
    emu.test_autogrid_snapped_faces(hip_lib)


def test_spheres_cylinders_and_two_tiles(hip_lib):
    emu.spheres(hip_lib)
    emu.cylinders(hip_lib)
    emu.test_two_x_tiles(hip_lib)


def test_fallbacks(hip_lib):
    for kind in ("polyslab", "medium2d", "kerr"):
        emu.test_fallback(hip_lib, kind)


def test_rest_of_set_up_and_web_run(hip_lib):
    emu.set_up(hip_lib)
    emu.run_both(hip_lib)


def test_renamed_axes_and_recursive_grids(hip_lib):
    for shift in (0, 1, 2):
        emu.test_renamed_axes(hip_lib, shift)
    emu.test_symmetric_and_pmc_plus_grids(hip_lib)


def test_interface_refusals(hip_lib, monkeypatch, tmp_path):
    emu.interface_refusals(hip_lib)
    emu.test_device_path_without_a_library(monkeypatch, tmp_path)
