"""The engine against the fp64 oracle NODE BY NODE, from dense random states (tests/dense_state.py; docs/history/DENSE_STATE.md), on
the CPU emulator: every entry of ``cases.CASES`` at its default shape, ``pml_box`` / ``media_mix`` over two x tiles with a body across
the seam, the graded grid with its graded axis on x, y and z under every axis renaming, four cases at three times their size (where
the runs do take step pairs); K = 1, 2 and 6 steps through the fused single steps, the two-pass kernels and step pairs.  The bar of
a case and K is MARGIN x what the fp32 oracle itself is off the fp64 oracle by, under the same measure.

The sensitivity tests need no library: a relative 1e-3 planted in ONE coefficient of an oracle instance must stand at 4 x the bar or
more, at the planted node or plane — that is what keeps the bar honest."""
import numpy as np
import pytest

import dense_state as ds
from cases import CASES

def _engine_vs_oracle(label, path, lib, shift=0, ks=ds.KS):
    case = ds.case(label)
    for K in ks:
        if path == "pairs" and K == 1:
            continue
        got = ds.run_engine(case.spec, lib, case.state, K, path, axis_shift=shift)
        case.check(got, K, f"{path} axis_shift={shift}")
        if path != "pairs":
            assert got.pairs == 0
        elif K == 6 and ds.TAKES_PAIRS.get(label) == shift:
            assert got.pairs >= 2 and got.why == 0, (label, got.pairs, got.why)
            assert label not in ds.SHELL2 or got.shell2_pairs == got.pairs, (label, got.pairs, got.shell2_pairs)


@pytest.mark.parametrize("path", ds.PATHS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_every_node_of_every_case_vs_oracle(name, path, emu_lib):
    _engine_vs_oracle(name, path, emu_lib)


@pytest.mark.parametrize("path", ds.PATHS)
@pytest.mark.parametrize("label", sorted(ds.SEAM))
def test_two_x_tiles_with_a_body_across_the_seam(label, path, emu_lib):
    assert ds.case(label).spec.shape[0] > ds.X_TILE + 8
    _engine_vs_oracle(label, path, emu_lib)


@pytest.mark.parametrize("shift", (0, 1, 2))
@pytest.mark.parametrize("label", sorted(ds.GRADED))
def test_graded_axis_on_every_axis_under_every_renaming(label, shift, emu_lib):
    for path in ds.PATHS:
        _engine_vs_oracle(label, path, emu_lib, shift)


@pytest.mark.parametrize("label", sorted(ds.TIMES3))
def test_three_times_the_size_through_pairs(label, emu_lib):
    """(the single-step paths of these shapes: the device module; here the pairs, which the default shapes are too small for)"""
    _engine_vs_oracle(label, "pairs", emu_lib, ks=(6,))


# ---- sensitivity: oracle against oracle ------------------------------------------------------------------------------------------
def _surface_cell(spec, c):
    """(i, j, k) of a cell of E component c inside a non-PEC body with another medium next to it, away from the grid's faces"""
    m = spec.mat_idx[c]
    nz, ny, nx = m.shape
    for k in range(2, nz - 2):
        for j in range(2, ny - 2):
            for i in range(2, nx - 2):
                if m[k, j, i] > 1 and not spec.media[m[k, j, i]].pec and (m[k - 1:k + 2, j - 1:j + 2, i - 1:i + 2] != m[k, j, i]).any():
                    return (i, j, k)
    raise AssertionError("no body surface")


def _dispersive(spec):
    return next(i for i, med in enumerate(spec.media) if len(med.poles))


def _plants():
    """(id, label, K, plant, check of the worst node's (comp, (i, j, k))).  K is the smallest number of steps after which the coefficient
    has acted on a dense state: 1 for what multiplies a field or a difference, 2 for what multiplies psi (zero before the first step);
    in the layers more steps only damp the planted node under its neighbours' scale.  Bodies and graded steps: K = 6."""
    out = []
    mm = ds.case("media_mix").spec
    cell = _surface_cell(mm, 2)
    out.append(("cb_one_surface_cell", "media_mix", 6, ds.plant_cb(2, cell), lambda w, cell=cell: w.comp == "Ez" and w.index == cell))
    pb = ds.case("pml_box").spec
    for a in range(3):
        i_lo, i_hi = 1, pb.shape[a] - 2                     # the second layer from outside, low face / high face
        for tab, i in (("c_e", i_lo), ("b_h", i_hi), ("kinv_e", i_hi)):
            out.append((f"{tab}_{'xyz'[a]}", "pml_box", 2, ds.plant_pml(a, tab, i),
                        lambda w, a=a, i=i, h=tab.endswith("h"): w.index[a] == i and (w.comp[0] == "H") == h))
    n = ds.case("graded_x").spec.shape[0]
    out.append(("inv_primal_last", "graded_x", 6, ds.plant_inv_step(0, False, n - 1), lambda w, n=n: w.index[0] == n - 1))
    out.append(("inv_dual_first", "graded_x_pmc", 6, ds.plant_inv_step(0, True, 0), lambda w: w.index[0] == 0 and w.comp in ("Ey", "Ez")))
    ab = ds.case("absorber_odd_rows").spec
    node = (ab.shape[0] - 2, 3, 1)                          # in the x+ and the z- layers at once
    out.append(("absorber_factor", "absorber_odd_rows", 1, ds.plant_absorber(1, node), lambda w, node=node: w.comp == "Ey" and w.index == node))
    med = _dispersive(mm)
    out.append(("ade_pair", "media_mix", 6, ds.plant_ade(med),
                lambda w, med=med: w.comp[0] == "E" and mm.mat_idx["xyz".index(w.comp[1])][w.index[2], w.index[1], w.index[0]] == med))
    return out


PLANTS = _plants()


@pytest.mark.parametrize("pid,label,K,plant,named", PLANTS, ids=[p[0] for p in PLANTS])
def test_a_planted_per_mille_stands_four_bars_high_at_its_node(pid, label, K, plant, named):
    case = ds.case(label)
    ref = case.ref(K)
    got = ds.run_oracle(case.spec, case.state, K, plant=plant)
    w = ds.worst_of(ds.measure_fields(case.spec, case.state, case.excluded, ref, got))
    bar = case.bar(K)
    print(f"[dense] planted {pid} in {label}, K={K}: per node {w.value:.3e} = {w.value / bar:.0f} x the bar {bar:.3e} at {w.at} | "
          f"whole-array rel-L2 {ds.rel_l2(ref, got):.3e} (run_case's bar: 2e-5)")
    assert w.value >= 4 * bar, (pid, w.value, bar)
    assert named(w), (pid, str(w))


def test_the_state_is_dense_and_admissible():
    """no node at rest, no outlier; pinned nodes are zero on both sides and are the only nodes left out"""
    for label in ("media_mix", "pml_box", "bloch_box", "pmc_plus_mix", "pec_box"):
        case = ds.case(label)
        inside = ds.mirror_crop(case.spec)
        for c in range(6):
            f, ex = case.state[c], case.excluded[c]
            assert f.dtype == (np.complex64 if case.spec.bloch is not None else np.float32)
            assert (f[ex] == 0).all() and (f[~ex] != 0).all(), (label, c)
            live = np.abs(f[~ex]) * (ds.ETA0 if c >= 3 else 1.0)
            assert live.max() < 6 * np.sqrt(np.mean(live ** 2)), (label, c)       # (white noise after six steps: 65 - 200 x rms)
            if c >= 3:
                assert not ex[inside].any(), (label, c)                           # H is pinned nowhere
        assert (case.share == 0) == (label == "bloch_box"), (label, case.share)
