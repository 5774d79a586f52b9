"""Every listed instantiation of the two-step sweep (fused2_step_kernel<LB, OPT>: one piece of gfx950 code per pair of the table
FDTD_F2_LIST_ALL — its own launch bound, register budget, LDS size, spills) on the device, at the scenarios of tests/sweep_matrix.py:
the run equals single steps of the same library bit for bit, fields and records, and launched exactly the (LB, OPT, W) the case was
written to reach (fdtd_get_sweep_words); once per scenario the pairs run is held to the fp64 oracle.  The closing test prints the
table with the cases that launched each pair and fails on a listed pair without one."""
import pytest

import sweep_matrix as M

pytestmark = pytest.mark.gpu

LAUNCHED = {}            # (LB, OPT) -> the cases that launched it and passed


@pytest.mark.parametrize("name", sorted(M.SCENARIOS))
def test_listed_instantiations_equal_single_steps_on_the_device(name, hip_lib):
    M.check_scenario(name, hip_lib, False, LAUNCHED)


def test_every_listed_instantiation_has_a_case_on_the_device(hip_lib):
    table = M.check_table(hip_lib, LAUNCHED)
    assert len(table) >= 110
