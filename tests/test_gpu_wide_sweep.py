"""The wide-table form of the single-step fused sweep on the device: the scenarios and comparisons of tests/wide_sweep_case.py that
tests/test_emu_wide_sweep.py runs on the CPU emulator.  The fused single steps and the two-pass kernels perform the same IEEE
operations (narrow table: tests/test_gpu_parity.py, and test_narrow_fused_equals_two_pass_on_the_seam_grid here), so the wide sweep
is held to wide VARIANT_ZMARCH bit for bit, and to the fp64 oracle at the bar of tests/test_wide_media.py."""
import numpy as np
import pytest

import wide_sweep_case as W
from tidy3d_amd import engine, lib as L
from tidy3d_amd.discretize import discretize
from tidy3d_amd.engine import HipEngine
from test_wide_media import wide_sim

pytestmark = pytest.mark.gpu

# rows per workgroup -> launch bound of the instantiation: 3 rows + halo = 256 threads, 7 -> 512, 15 -> 1024 (PML = 0 only)
ROWS = {"a": (3, 7), "b": (3, 7), "c": (3, 7, 15), "d": (3, 7), "e": (3,), "f": (3,), "g": (3, 7, 15)}


@pytest.fixture(scope="module")
def two_pass(hip_lib):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = W.run(W.scenario(name).spec, hip_lib, variant=L.VARIANT_ZMARCH)
            assert cache[name].stats.fused2_off_reason == W.F2_OFF_VARIANT and cache[name].stats.fused_kernel_launches == 0
        return cache[name]
    return get


@pytest.mark.parametrize("name,rows", [(n, r) for n in W.SCENARIOS for r in ROWS[n]])
def test_wide_sweep_against_oracle_and_two_pass(hip_lib, two_pass, name, rows):
    spec = W.scenario(name).spec
    out = W.run(spec, hip_lib, options={L.OPT_ROWS: rows})
    W.assert_fused_wide(out, spec.n_steps)
    assert out.stats.fused2_off_reason == W.F2_OFF_WIDE_TABLE
    if rows == ROWS[name][0]:
        W.assert_oracle(out, name)
    W.assert_same_bits(out, two_pass(name), (name, rows, "fused wide vs two-pass"))


def test_wide_sweep_with_memory_hints_and_slab_kernel_cpml(hip_lib, two_pass):
    spec = W.scenario("a").spec
    for opts in ({L.OPT_MEM_HINTS: 1}, {L.OPT_PML_FUSED: 0}, {L.OPT_PML_SPLIT: 1}):
        out = W.run(spec, hip_lib, options=opts)
        W.assert_fused_wide(out, spec.n_steps)
        W.assert_same_bits(out, two_pass("a"), opts)


def test_narrow_fused_equals_two_pass_on_the_seam_grid(hip_lib):
    spec = discretize(wide_sim(W.SEAM, 24), n_steps=W.STEPS["b"]).spec
    assert len(spec.media) <= 1023
    a = W.run(spec, hip_lib, options=W.SINGLE_STEPS)
    b = W.run(spec, hip_lib, variant=L.VARIANT_ZMARCH)
    assert a.stats.fused_kernel_launches >= spec.n_steps and b.stats.fused_kernel_launches == 0
    W.assert_same_bits(a, b, "narrow fused vs two-pass")


@pytest.mark.parametrize("kind,how", [(k, h) for k in ("layers", "planted") for h in sorted(W.WIDENED)])
def test_same_bits_as_the_narrow_table(hip_lib, kind, how):
    spec = W.narrow_spec(kind)
    narrow = W.run(spec, hip_lib, options=W.SINGLE_STEPS)
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
    wide = W.run(wide_spec, hip_lib, options=W.SINGLE_STEPS)
    W.assert_fused_wide(wide, spec.n_steps)
    W.assert_same_bits(wide, narrow, (kind, how))


def test_planted_rows_are_felt(hip_lib, two_pass):
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
        other = W.run(dataclasses.replace(spec, mat_idx=mat), hip_lib, variant=L.VARIANT_ZMARCH)
        assert any(not np.array_equal(other.fields[c], ref.fields[c]) for c in range(6)), triple


def test_selection(hip_lib):
    spec = W.scenario("a").spec
    with HipEngine(spec, lib=hip_lib, variant=L.VARIANT_FUSED) as e:
        assert e.variant == L.VARIANT_FUSED
        st = e.run()
        assert st.fused2_pairs == 0 and st.fused2_off_reason == W.F2_OFF_WIDE_TABLE
    with HipEngine(spec, lib=hip_lib) as e:                                    # AUTO below 2^20 cells
        assert e.variant == L.VARIANT_ZMARCH


def test_auto_just_above_the_size_threshold(hip_lib):
    """272 x 64 x 64 = 1.1 M cells, 20 steps: VARIANT_AUTO follows engine.WIDE_SWEEP_AUTO (the 320^3 measurement,
    docs/history/WIDE_SWEEP.md); whichever it takes gives the bits of the two-pass kernels, and so does the explicit wide sweep."""
    spec = discretize(wide_sim((272, 64, 64), 32, eps_span=2.0, sig_span=10.0), n_steps=20).spec
    assert len(spec.media) > 1023 and int(np.prod(spec.shape)) >= 1 << 20
    ref = W.run(spec, hip_lib, variant=L.VARIANT_ZMARCH)
    auto = W.run(spec, hip_lib, variant=L.VARIANT_AUTO)
    assert auto.variant == (L.VARIANT_FUSED if engine.WIDE_SWEEP_AUTO else L.VARIANT_ZMARCH)
    W.assert_same_bits(auto, ref, "AUTO vs two-pass")
    fused = W.run(spec, hip_lib)
    W.assert_fused_wide(fused, spec.n_steps)
    W.assert_same_bits(fused, ref, "fused wide vs two-pass")


def test_lifecycle(hip_lib):
    W.lifecycle(hip_lib)
