"""The device against the fp64 oracle NODE BY NODE, from dense random states (tests/dense_state.py; docs/history/DENSE_STATE.md): the
helper, the measure and the bars of tests/test_emu_dense_state.py — the floors come from the oracle and know nothing of the device.
Every entry of ``cases.CASES`` at its default shape, ``pml_box`` / ``media_mix`` over two x tiles with a body across the seam at cell
256, and ``pml_box``, ``drude_in_pml``, ``au_array``, ``lorentz_sphere`` at three times their size (several workgroups per axis,
dispersive cells running into the layers); K = 1, 2 and 6 steps through the fused single steps, the two-pass kernels and step pairs."""
import pytest

import dense_state as ds
from cases import CASES

pytestmark = pytest.mark.gpu

LABELS = sorted(CASES) + sorted(ds.SEAM) + sorted(ds.TIMES3)


@pytest.mark.parametrize("path", ds.PATHS)
@pytest.mark.parametrize("label", LABELS)
def test_every_node_vs_oracle_on_device(label, path, hip_lib):
    case = ds.case(label)
    for K in ds.KS:
        if path == "pairs" and K == 1:
            continue
        got = ds.run_engine(case.spec, hip_lib, case.state, K, path)          # (the engine is created and closed in there)
        case.check(got, K, path)
        if path != "pairs":
            assert got.pairs == 0
        elif K == 6 and ds.TAKES_PAIRS.get(label) == 0:
            assert got.pairs >= 2 and got.why == 0, (label, got.pairs, got.why)
            assert label not in ds.SHELL2 or got.shell2_pairs == got.pairs, (label, got.pairs, got.shell2_pairs)
