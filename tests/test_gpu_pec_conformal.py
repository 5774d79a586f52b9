"""PEC-conformal boundaries (SubpixelSpec.pec = PECConformal) on the device, through the C ABI: the scenarios of
tests/pec_conformal_case.py against the fp64 ConformalOracle (2e-5 rel-L2 per field, fused single steps and two-pass kernels, equal
bits between them wherever the plain sweeps of the same spec have them; the first scenario under all three axis renamings), the off
reason, the handle's lifecycle, and the device against the emulator's record (tests/golden/pec_conformal/emulator_k7.npz, kept
current by tests/test_emu_pec_conformal.py): at most 4 fp32 ulps of the largest listed value.  The operator tests, the front end and
the emulator's pins are in tests/test_emu_pec_conformal.py."""
import pytest

from tidy3d_amd import lib as L

import pec_conformal_case as pc
from test_emu_pec_conformal import lifecycle, off_reason

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("K", pc.KS)
@pytest.mark.parametrize("run_label", list(pc.RUNS))
def test_scenario_matches_the_conformal_oracle(run_label, K, hip_lib):
    label, shift = pc.RUNS[run_label]
    assert pc.scenario(label).visibility(1) >= pc.VISIBLE
    _, got = pc.check_run(hip_lib, run_label, K, what="device ")
    if K == 7 and shift == 0 and label in pc.SCENARIOS:
        pc.check_against_emulator_record(label, got["fused"].fields)


def test_off_reason(hip_lib):
    off_reason(hip_lib)


@pytest.mark.parametrize("variant", ["fused", "twopass"])
def test_lifecycle(variant, hip_lib):
    lifecycle(hip_lib, L.VARIANT_ZMARCH if variant == "twopass" else L.VARIANT_AUTO)
