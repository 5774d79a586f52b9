"""Live source injection against the fp64 oracle NODE BY NODE on the device (tests/source_state.py; docs/history/SOURCE_STATE.md): the
scenarios, the protocol and the bars of tests/test_emu_source_state.py — the floors come from the oracle and know nothing of the device."""
import pytest

import dense_state as ds
import source_state as ss

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("path", ds.PATHS)
@pytest.mark.parametrize("label", list(ss.SCENARIOS))
def test_live_sources_at_every_node_vs_oracle_on_device(label, path, hip_lib):
    ss.engine_vs_oracle(label, path, hip_lib, "gpu")
