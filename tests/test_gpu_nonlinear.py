"""Kerr media (Medium.nonlinear_spec with NonlinearSusceptibility models) on the device, through the C ABI: the five scenarios of
tests/nonlinear_case.py against the fp64 NonlinearOracle (2e-5 rel-L2 per field, fused single steps and two-pass kernels, equal bits
between them, num_iters 1 and 5), chi3 = 0, the Jacobi order, the off reason, the handle's lifecycle, and the device against the
emulator's record (tests/golden/nonlinear/emulator_k7.npz, kept current by tests/test_emu_nonlinear.py): at most 4 fp32 ulps of the
largest listed value.  The emulator's pins, the entry points and the physics pin are in tests/test_emu_nonlinear.py."""
import numpy as np
import pytest

from tidy3d_amd import lib as L

import dense_state as ds
import nonlinear_case as nc
from test_emu_nonlinear import lifecycle, off_reason

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("num_iters", nc.ITERS)
@pytest.mark.parametrize("K", nc.KS)
@pytest.mark.parametrize("label", nc.Scenario.all_labels())
def test_scenario_matches_the_nonlinear_oracle(label, K, num_iters, hip_lib):
    sc = nc.scenario(label)
    assert sc.visibility(K) >= 100 * nc.BAR
    _, got = nc.check_scenario(hip_lib, label, K, num_iters, what="device ")
    if K == 7 and num_iters == 5 and label in nc.SCENARIOS:
        nc.check_against_emulator_record(label, got["fused"].fields)


def test_iterations_are_counted(hip_lib):
    """a kernel that iterated once would match the num_iters = 1 reference and miss this one by more than ten times the bar"""
    sc = nc.scenario("pec_box_blocks")
    got = sc.run(hip_lib, 7, "fused", 5)
    assert sc.listed_diff(sc.ref(7, 5), sc.ref(7, 1)) > 10 * nc.BAR
    assert sc.listed_diff(sc.ref(7, 5), got.fields) <= nc.BAR < sc.listed_diff(sc.ref(7, 1), got.fields)


@pytest.mark.parametrize("label", list(nc.SCENARIOS))
def test_chi3_zero_gives_the_bits_of_the_plain_spec(label, hip_lib):
    sc = nc.scenario(label)
    zero = sc.run(hip_lib, 7, "fused", scale=0.0)
    plain = sc.run(hip_lib, 7, "fused", plain=True)
    for c in range(6):
        assert np.array_equal(zero.fields[c], plain.fields[c]), (label, ds.COMP[c])


def test_jacobi_order(hip_lib):
    sc = nc.scenario("pec_box_blocks")
    a, b = sc.run(hip_lib, 7, "fused"), sc.run(hip_lib, 7, "fused", reverse=True)
    for c in range(6):
        assert np.array_equal(a.fields[c], b.fields[c]), ds.COMP[c]


def test_off_reason(hip_lib):
    off_reason(hip_lib)


@pytest.mark.parametrize("variant", ["fused", "twopass"])
def test_lifecycle(variant, hip_lib):
    lifecycle(hip_lib, L.VARIANT_ZMARCH if variant == "twopass" else L.VARIANT_AUTO)
