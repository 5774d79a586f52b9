"""Live source injection against the fp64 oracle NODE BY NODE, on the CPU emulator (tests/source_state.py; docs/history/SOURCE_STATE.md):
a warm-up to the step at which the case injects most, a dense state of the injections' amplitude over all six fields, K = 1, 2 and 6
steps through the fused single steps, the two-pass kernels and step pairs; every node and record element under 8 x what the fp32 oracle
is off the fp64 oracle by.  The conditions on the reference (every list live, no listed node excluded) are asserted when a case is built.

The planted deviations need no library: a relative 1e-3 in one weight or coefficient, a moved index or a dropped entry in ONE oracle
instance must stand at 4 x the bar or more and be named — list, side and entry — by the failure sentence."""
import pytest

import dense_state as ds
import source_state as ss


@pytest.mark.parametrize("path", ds.PATHS)
@pytest.mark.parametrize("label", list(ss.SCENARIOS))
def test_live_sources_at_every_node_vs_oracle(label, path, emu_lib):
    ss.engine_vs_oracle(label, path, emu_lib, "emu")


def test_the_two_boxes_differ(emu_lib):
    """normal and oblique incidence differ in W, in A, in every floor and in every engine figure: the sources do act on what is measured"""
    a, b = ss.case("tfsf_box"), ss.case("tfsf_angled_box")
    assert a.W != b.W and a.A != b.A
    for K in ds.KS:
        assert a.floor(K)[0].value != b.floor(K)[0].value, K
        fa, fb = (ds.measure(c.spec, c.state, c.excluded, c.ref(K), c.run(emu_lib, K, "fused"))[0].value for c in (a, b))
        assert fa != fb, (K, fa, fb)


def test_a_list_that_ends_inside_a_pair(emu_lib):
    """the first list's last step falls on the first step of a would-be pair in one of the two parities: that pair must not go out with
    the node table (the H-side terms of its second step come from the table row of ALL lists), so it is paged — or single steps"""
    runs = [ss.engine_vs_oracle(label, "pairs", emu_lib, "emu", ks=(6,)) for label in ("spent_list", "spent_list_even")]
    assert ss.case("spent_list").W == ss.case("spent_list_even").W
    assert any(r.src_paged_pairs >= 1 or r.pairs < 2 for r in runs), [(r.pairs, r.src_paged_pairs) for r in runs]


@pytest.mark.parametrize("pid", ss.PLANT_IDS)
def test_a_planted_deviation_stands_four_bars_high_and_is_named(pid):
    label, K, plant, clause, entry, aux = ss.plant_of(pid)
    case = ss.case(label)
    ref, got = case.ref(K), case.planted(K, plant)
    w = ds.worst_of(ds.measure_fields(case.spec, case.state, case.excluded, ref, got))
    bar = case.bars(K)[0]
    # the same plant under the protocol that starts at step 0 (recorded, not asserted: it shows the gap)
    cold = ds.Case(label, case.spec)
    w0 = ds.worst_of(ds.measure_fields(cold.spec, cold.state, cold.excluded, cold.ref(K), ds.run_oracle(cold.spec, cold.state, K, plant=plant)))
    print(f"[source] planted {pid} in {label}, K={K}: per node {w.value:.3e} = {w.value / bar:.1f} x the bar {bar:.3e} at {w.at} | "
          f"whole-array rel-L2 {ds.rel_l2(ref, got):.3e} (run_case's bar: 2e-5) | from step 0: {w0.value:.3e} = {w0.value / cold.bar(K):.3f} x its bar")
    assert w.value >= 4 * bar, (pid, w.value, bar)
    assert "listed: " + clause in w.at, (pid, str(w))
    entries, reads = ss.named(w.at, clause)
    assert entry is None or entry in entries, (pid, entry, str(w))
    assert aux is None or aux in reads, (pid, aux, str(w))
