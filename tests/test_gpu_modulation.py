"""Time-modulated media (Medium.modulation_spec) on the device, through the C ABI: the five scenarios of tests/modulation_case.py
against the fp64 ModulatedOracle (2e-5 rel-L2 per field, fused single steps and two-pass kernels, equal bits between them wherever
the plain sweeps of the same spec have them), the off reason, the handle's lifecycle, and the device against the emulator's record
(tests/golden/modulation/emulator_k7.npz, kept current by tests/test_emu_modulation.py): at most 4 fp32 ulps of the largest listed
value.  The emulator's pins, the front end and the physics pin are in tests/test_emu_modulation.py."""
import dataclasses

import pytest

import tidy3d_amd.schema as td
from tidy3d_amd import lib as L
from tidy3d_amd.discretize import discretize
from tidy3d_amd.engine import HipEngine

import modulation_case as mc
from test_emu_modulation import lifecycle

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("K", mc.KS)
@pytest.mark.parametrize("label", mc.Scenario.all_labels())
def test_scenario_matches_the_modulated_oracle(label, K, hip_lib):
    sc = mc.scenario(label)
    assert sc.visibility(K) >= 100 * mc.BAR
    _, got = mc.check_scenario(hip_lib, label, K, what="device ")
    if K == 7 and label in mc.SCENARIOS:
        mc.check_against_emulator_record(label, got["fused"].fields)


def test_off_reason(hip_lib):
    sim = mc._box_sim((128, 128, 64), td.BoundarySpec(x=mc._pec(), y=mc._pec(), z=mc._pec()),
                      [td.Structure(geometry=td.Box(center=(0, 0, 0), size=(0.4, 0.4, 0.4)), medium=mc.eps_modulated())])
    spec = discretize(sim, n_steps=4).spec
    spec.decay_every = 0
    with HipEngine(spec, lib=hip_lib) as e:
        st = e.run(4)
    assert int(st.fused2_pairs) == 0 and int(st.fused2_off_reason) == 15
    with HipEngine(dataclasses.replace(spec, modulation=[]), lib=hip_lib) as e:       # the same grid without the lists does take pairs
        assert int(e.run(4).fused2_pairs) == 2


@pytest.mark.parametrize("variant", ["fused", "twopass"])
def test_lifecycle(variant, hip_lib):
    lifecycle(hip_lib, L.VARIANT_ZMARCH if variant == "twopass" else L.VARIANT_AUTO)
