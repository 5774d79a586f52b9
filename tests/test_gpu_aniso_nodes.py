"""The fully anisotropic coupling lists across periodic and Bloch faces on the device, through the C ABI: the scenarios, step counts,
paths, floors and bars of tests/test_emu_aniso_nodes.py — they know nothing of the device (docs/history/ANISO_WRAPS.md)."""
import pytest

import aniso_case as ac

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("K", ac.KS)
@pytest.mark.parametrize("label", ac.Scenario.all_labels())
def test_every_node_matches_the_oracle(label, K, hip_lib):
    ac.check_scenario(hip_lib, label, K, what="device ")
