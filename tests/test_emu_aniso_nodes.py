"""The fully anisotropic coupling lists across periodic and Bloch faces on the HIP-on-CPU emulator: every scenario of
tests/aniso_case.py, 1, 2 and 7 steps through the fused single steps and the two-pass kernels, every node under 8 x the floor of the
fp32 oracle of the same scenario and K (docs/history/ANISO_WRAPS.md).  The device runs the same in tests/test_gpu_aniso_nodes.py."""
import pytest

import aniso_case as ac


@pytest.mark.parametrize("K", ac.KS)
@pytest.mark.parametrize("label", ac.Scenario.all_labels())
def test_every_node_matches_the_oracle(label, K, emu_lib):
    ac.check_scenario(emu_lib, label, K, what="emulator ")
