"""Every listed instantiation of the two-step sweep (fused2_step_kernel<LB, OPT>, the table FDTD_F2_LIST_ALL read back through
fdtd_sweep_table) against single steps of the same library on the CPU emulator, at the scenarios of tests/sweep_matrix.py: bit for
bit, with the (LB, OPT, W) the run launched (fdtd_get_sweep_words) held to the ones the case was written to reach; once per scenario
to the fp64 oracle.  The closing test holds the matrix to the table: a listed pair without a case fails it.  (The emulator compiles
non-temporal stores and launch bounds away: tests/test_gpu_sweep_table.py runs the same cases on the device.)"""
import pytest

import sweep_matrix as M

LAUNCHED = {}            # (LB, OPT) -> the cases of this process that launched it and passed


@pytest.mark.parametrize("name", sorted(M.SCENARIOS))
def test_listed_instantiations_equal_single_steps(name, emu_lib):
    M.check_scenario(name, emu_lib, True, LAUNCHED)


def test_every_listed_instantiation_has_a_case(emu_lib):
    """(the scenarios may have run in other worker processes: the condition is on what the cases are written to reach — each of them
    fails unless its run launched exactly that)"""
    table = M.check_table(emu_lib, LAUNCHED)
    assert len(table) >= 110
