"""The wide-table form of the single-step fused sweep on the CPU emulator (scenarios and comparisons: tests/wide_sweep_case.py).

Precondition of the comparison with the two-pass kernels, checked here on the emulator: with a NARROW table (<= 1022 media) the
fused single steps and VARIANT_ZMARCH give the same bits on the two-tile grid (test_narrow_fused_equals_two_pass_on_the_seam_grid);
the wide sweep is therefore held to the same: bit-identical to wide ZMARCH on (a) ... (g)."""
import numpy as np
import pytest

import wide_sweep_case as W
from tidy3d_amd import lib as L
from tidy3d_amd.discretize import discretize
from tidy3d_amd.engine import HipEngine
from test_wide_media import wide_sim

# rows per workgroup -> the launch bound of the instantiation: 3 rows + halo = 256 threads, 7 -> 512, 15 -> 1024 (PML = 0 only)
ROWS = {"a": (3, 7), "b": (3,), "c": (3, 7, 15), "d": (3, 7), "e": (3,), "f": (3,), "g": (3, 15)}


@pytest.fixture(scope="module")
def two_pass(emu_lib):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = W.run(W.scenario(name).spec, emu_lib, variant=L.VARIANT_ZMARCH)
            assert cache[name].stats.fused2_off_reason == W.F2_OFF_VARIANT and cache[name].stats.fused_kernel_launches == 0
        return cache[name]
    return get


@pytest.mark.parametrize("name,rows", [(n, r) for n in W.SCENARIOS for r in ROWS[n]])
def test_wide_sweep_against_oracle_and_two_pass(emu_lib, two_pass, name, rows):
    spec = W.scenario(name).spec
    out = W.run(spec, emu_lib, options={L.OPT_ROWS: rows})
    W.assert_fused_wide(out, spec.n_steps)
    assert out.stats.fused2_off_reason == W.F2_OFF_WIDE_TABLE
    if rows == ROWS[name][0]:
        W.assert_oracle(out, name)
    W.assert_same_bits(out, two_pass(name), (name, rows, "fused wide vs two-pass"))


def test_wide_sweep_with_memory_hints_and_slab_kernel_cpml(emu_lib, two_pass):
    # the memory-hint instantiations (HINT = 128 with CPML) and the CPML recursions left to the slab kernels (PML = 0 sweep + pml_*_kernel with m4b)
    spec = W.scenario("a").spec
    for opts in ({L.OPT_MEM_HINTS: 1}, {L.OPT_PML_FUSED: 0}, {L.OPT_PML_SPLIT: 1}):
        out = W.run(spec, emu_lib, options=opts)
        W.assert_fused_wide(out, spec.n_steps)
        W.assert_same_bits(out, two_pass("a"), opts)


def test_narrow_fused_equals_two_pass_on_the_seam_grid(emu_lib):
    # test 3's precondition: <= 1022 media on scenario (b)'s grid
    spec = discretize(wide_sim(W.SEAM, 24), n_steps=W.STEPS["b"]).spec
    assert len(spec.media) <= 1023
    a = W.run(spec, emu_lib, options=W.SINGLE_STEPS)
    b = W.run(spec, emu_lib, variant=L.VARIANT_ZMARCH)
    assert a.stats.fused_kernel_launches >= spec.n_steps and b.stats.fused_kernel_launches == 0
    W.assert_same_bits(a, b, "narrow fused vs two-pass")


@pytest.mark.parametrize("kind,how", [(k, h) for k in ("layers", "planted") for h in sorted(W.WIDENED)])
def test_same_bits_as_the_narrow_table(emu_lib, kind, how):
    spec = W.narrow_spec(kind)
    narrow = W.run(spec, emu_lib, options=W.SINGLE_STEPS)
    assert narrow.stats.fused2_pairs == 0 and narrow.stats.fused_kernel_launches >= spec.n_steps
    n_table, first = W.WIDENED[how]
    wide_spec = W.widened(spec, n_table, first)
    cls = W.segment_classes(wide_spec)
    if kind == "layers":          # rows end in PEC padding: every segment is mixed under any table
        assert cls["background"] == cls["packed"] == cls["uniform_wide_index"] == 0
    elif first is None:           # only padded: the planted rows keep packed words of non-background triples
        assert cls["packed"] > 0 and cls["background"] > 0 and cls["uniform_wide_index"] == 0 and cls["mixed"] > 0
    else:                         # remapped: the planted rows are uniform and name indices > 1023
        assert cls["packed"] == 0 and cls["uniform_wide_index"] > 0 and cls["background"] > 0
    wide = W.run(wide_spec, emu_lib, options=W.SINGLE_STEPS)
    W.assert_fused_wide(wide, spec.n_steps)
    W.assert_same_bits(wide, narrow, (kind, how))


def test_planted_rows_are_felt(emu_lib, two_pass):
    """the comparisons above judge the row-segment words only if the planted rows matter: exchanging the E_y and E_z indices of the
    packed triple, or of the triple above 1023, changes the two-pass result"""
    import dataclasses
    spec = W.scenario("g").spec
    ref = two_pass("g")
    for triple in (W.PLANTED_WIDE[0], W.PLANTED_WIDE[1]):
        mat = np.array(spec.mat_idx)
        rows = np.all(mat[0] == triple[0], axis=(0, 2)) & np.all(mat[1] == triple[1], axis=(0, 2)) & np.all(mat[2] == triple[2], axis=(0, 2))
        assert rows.sum() == 1
        mat[1][:, rows, :], mat[2][:, rows, :] = triple[2], triple[1]
        other = W.run(dataclasses.replace(spec, mat_idx=mat), emu_lib, variant=L.VARIANT_ZMARCH)
        assert any(not np.array_equal(other.fields[c], ref.fields[c]) for c in range(6)), triple


def test_selection(emu_lib, caplog):
    spec = W.scenario("a").spec
    with HipEngine(spec, lib=emu_lib, variant=L.VARIANT_FUSED) as e:          # (raised ValueError before the wide sweep existed)
        assert e.variant == L.VARIANT_FUSED
        st = e.run()
        assert st.fused2_pairs == 0 and st.fused2_off_reason == W.F2_OFF_WIDE_TABLE
        assert L.F2_OFF_REASONS[W.F2_OFF_WIDE_TABLE].startswith("wide material table")
    with HipEngine(spec, lib=emu_lib) as e:                                    # AUTO below 2^20 cells
        assert e.variant == L.VARIANT_ZMARCH
    import logging
    import tidy3d_amd.schema as td
    per_z = W.scenario_sim("a").copy(boundary_spec=td.BoundarySpec(x=W.PEC, y=W.PEC, z=td.Boundary.periodic()))
    spec_z = discretize(per_z, n_steps=4).spec
    for v in (L.VARIANT_AUTO, L.VARIANT_FUSED):
        caplog.clear()
        with caplog.at_level(logging.WARNING, logger="tidy3d_amd"):
            with HipEngine(spec_z, lib=emu_lib, variant=v, force_comm=True) as e:  # a communicator handle keeps the two-pass kernels
                assert e.variant == L.VARIANT_ZMARCH
        said = any("VARIANT_FUSED was asked for" in r.getMessage() for r in caplog.records)
        assert said == (v == L.VARIANT_FUSED)            # asked for and not given: the engine says so


def test_auto_rule():
    from tidy3d_amd import engine
    assert not engine.wide_sweep_pays((1 << 20) - 1)
    assert engine.wide_sweep_pays(1 << 20) == engine.WIDE_SWEEP_AUTO


def test_lifecycle(emu_lib):
    W.lifecycle(emu_lib)
