"""The fully anisotropic coupling lists across periodic and Bloch faces, node by node — the reference side (CPU, no engine;
docs/history/ANISO_WRAPS.md): the oracle's Bloch factor pinned by a translation of its own cell, what keeps the measure of
``aniso_case.check_scenario`` honest (excluded share, no listed node excluded, the shapes and slots the scenarios hold between them), the
sentence a failure prints, and the planted deviations (clean fp64 oracle against an fp64 oracle whose spec has one slot, one wrap or one
weight changed).  The engine runs are in tests/test_emu_aniso_nodes.py and tests/test_gpu_aniso_nodes.py."""
import dataclasses

import numpy as np
import pytest

from oracle.fdtd_numpy import OracleFdtd

import aniso_case as ac
import dense_state as ds
import list_case as lc
import test_aniso_bloch as tab

PIN = 1e-12                   # of the largest value of the component: fp64 rounding over 150 steps (measured: 8e-15)


# ---------------------------------------------------------------------------------------------------------------- the oracle's own pin
@pytest.mark.parametrize("cell", ["bloch_xy_corner", "bloch_xyz_corner"])
def test_the_oracles_bloch_factor_is_a_translation(cell):
    """the corner cell, whose slots cross the Bloch faces, against its twin with the body in the middle, where the oracle runs the code it
    always ran: every node within 1e-12 of the largest value of its component after 150 steps"""
    make = {"bloch_xy_corner": lambda c: tab.wrapped_cell(center=c), "bloch_xyz_corner": lambda c: ac.corner_cell((16, 14, 10), ("bloch",) * 3, c)}[cell]
    fa, mapped, spec = ac.oracle_translation(make)
    assert spec.shape == ac.scenario(cell).spec.shape and len(ac.live_wraps(spec)) == len(ac.live_wraps(ac.scenario(cell).spec))
    worst = ac.node_agreement(fa, mapped)
    print(f"[pin] {cell} {spec.shape}, 150 steps, phases {' / '.join(f'{p:.3f}' for p in spec.bloch)} rad, {len(ac.live_wraps(spec))} live slots across a wrap: "
          "worst node per component " + " ".join(f"{ds.COMP[c]} {worst[c]:.1e}" for c in range(6)) + f" of the largest value (bar {PIN:g})")
    assert max(worst) <= PIN, worst
    # ... and the factor is what closes it: without the periods crossed the same cell misses by parts in ten
    bare = dataclasses.replace(spec, aniso=[dataclasses.replace(st, nbr_wrap=np.zeros_like(st.nbr_wrap)) for st in spec.aniso])
    o = OracleFdtd(bare)
    o.run()
    assert max(ac.node_agreement(o.E + o.H, mapped)) > 0.1


def test_periodic_faces_take_no_factor():
    """without Bloch phases the periods crossed change nothing: equal bits with and without ``nbr_wrap``"""
    sc = ac.scenario("periodic_xyz_corner")
    bare = dataclasses.replace(sc.spec, aniso=[dataclasses.replace(st, nbr_wrap=None) for st in sc.lists])
    for a, b in zip(sc.ref(2), sc._run(OracleFdtd, bare, 2)):
        assert not np.iscomplexobj(a) and np.array_equal(a, b)


def test_bloch_lists_without_wrap_signs_are_refused():
    """as the engine refuses them: the oracle does not run them with no factor"""
    spec = ac.scenario("bloch_xy_corner").spec
    o = OracleFdtd(dataclasses.replace(spec, aniso=[dataclasses.replace(st, nbr_wrap=None) for st in spec.aniso]))
    with pytest.raises(ValueError, match="wrap signs"):
        o.step()


# ---------------------------------------------------------------------------------------------------------------- inputs
def test_excluded_share_and_listed_nodes():
    for label in ac.Scenario.all_labels():
        sc = ac.scenario(label)
        print(f"[dense] aniso {label} {sc.spec.shape}: excluded {100 * sc.share:.2f} % (cap {100 * lc.SHARE_CAP:.0f} %), "
              f"{sum(len(s.ijk) for s in sc.lists)} listed nodes, none excluded, {len(ac.live_wraps(sc.spec))} live slots across a wrap")
        sc.check_inputs()


def test_scenarios_hold_tail_lanes_and_empty_and_wrapped_slots():
    for what, found in lc.presence(ac.Scenario).items():
        print(f"[dense] aniso: {what}: " + (", ".join(f"{label} {comp} ({n})" for label, comp, n in found) or "none"))
        assert found, what
    across = {label: ac.sign_sets(ac.scenario(label).spec) for label in ac.Scenario.all_labels() if label != "bloch_clear_pml_z"}
    assert any(one for one, _ in across.values()) and any(two for _, two in across.values())          # a slot across one axis, one across two
    # all six single-axis signs; of the twelve two-axis sign pairs the six the stencil can form (aniso_case.PAIRS) and no other
    for label in ("bloch_xyz_corner", "periodic_xyz_corner"):
        one, two = across[label]
        print(f"[dense] aniso {label}: crossings " + ", ".join(sorted(ac.sign_name([dict(k).get(a, 0) for a in range(3)]) for k in one | two)))
        assert one == ac.SINGLE and two == ac.PAIRS and len(two) == 6, (label, one, two)
    assert not len(ac.live_wraps(ac.scenario("bloch_clear_pml_z").spec))


def test_small_body_reads_the_wall():
    """``small_at_wall``: live slots that read pinned nodes of the z- wall, listed nodes whose slots are empty, none of them excluded"""
    sc = ac.scenario("small_at_wall")
    pinned = empty = 0
    for s in sc.lists:
        nbr = sc.slots_of(s)[0]
        for slot in range(8):
            ok = nbr[:, slot, 0] >= 0
            at = nbr[ok, slot]
            pinned += int(sc.excluded[s.nbr_comp[slot]][at[:, 2], at[:, 1], at[:, 0]].sum())
        empty += int((np.asarray(s.nbr_ijk)[:, :, 0] < 0).sum())
    print(f"[dense] aniso small_at_wall: {pinned} live slots read a pinned wall node, {empty} slots lie beyond the wall")
    assert pinned > 0 and empty > 0


def test_the_sentence_names_list_entry_slots_and_signs():
    sc = ac.scenario("bloch_xyz_corner")
    s = sc.lists[0]
    n, nbr = len(s.ijk), sc.slots_of(s)[0]
    w = np.where((nbr[:, :, 0] >= 0)[:, :, None], np.asarray(s.nbr_wrap, np.int64), 0)
    e = int(np.flatnonzero((np.abs(w).sum(axis=2) == 2).any(axis=1))[0])          # an entry with a slot across two axes
    said = sc.where(s.comp, s.ijk[e])
    signs = [ac.sign_name(v) for v in w[e] if v.any()]
    assert f"aniso list 0 (Ex), entry {e} of {n} (block {e // 256}, lane {e % 256})" in said, said
    assert f"{int((nbr[e, :, 0] < 0).sum())} of its 8 slots empty, {len(signs)} wrapped ({', '.join(signs)})" in said, said
    assert any(len(v) == 4 for v in signs), signs
    last = sc.where(s.comp, s.ijk[n - 1])
    assert n == 304 and "entry 303 of 304 (block 1, lane 47)" in last, last
    assert "not listed" in sc.where(0, (8, 7, 5))


# ---------------------------------------------------------------------------------------------------------------- planted deviations
def test_planted_deviations():
    """one change per run, in list 0 (Ex) of ``bloch_xyz_corner``; the entry: the one at the median of what the plant changes in the
    sum its node reads, from the reference alone (``aniso_case.slot_terms``)"""
    sc, n = ac.scenario("bloch_xyz_corner"), 0
    spec, s = sc.ref_spec(), sc.lists[0]
    assert s.comp == 0
    nbr = sc.slots_of(s)[0]
    live = nbr[:, :, 0] >= 0
    wrap = np.where(live[:, :, None], np.asarray(s.nbr_wrap, np.int64), 0)
    phases = np.asarray(spec.bloch)
    t, theta = ac.slot_terms(sc, s)
    size = np.abs(t)
    crossing, two = wrap.any(axis=2), np.abs(wrap).sum(axis=2) == 2

    def plant(name, e, slot, **change):
        return lc.stands(sc, f"{name}: slot {slot} of Ex entry {e} ({ac.sign_name(wrap[e, slot]) or 'inside'})", lc.replace_list(spec, "aniso", n, **change),
                       [(0, s.ijk[e])])
    # the conjugate factor; no factor; on a slot across two axes the list's own axis dropped
    e, q = lc.best(np.where(crossing, size * np.abs(1.0 - np.exp(-2j * theta)), 0.0))
    plant("wrap sign flipped", e, q, **ac.with_wrap(s, e, q, -wrap[e, q]))
    e, q = lc.best(np.where(crossing, size * np.abs(1.0 - np.exp(-1j * theta)), 0.0))
    plant("wrap set to 0", e, q, **ac.with_wrap(s, e, q, 0))
    e, q = lc.best(np.where(two, size * np.abs(1.0 - np.exp(-1j * wrap[:, :, 0] * phases[0])), 0.0))
    assert wrap[e, q, 0] == 1
    plant("x sign dropped", e, q, **ac.with_wrap(s, e, q, wrap[e, q] * (0, 1, 1)))
    # a slot one cell further along x (where that stays in the cell); a slot emptied
    moved = nbr.copy()
    moved[:, :, 0] += 1
    moved[~(live & (moved[:, :, 0] < spec.shape[0]))] = -1
    e, q = lc.best(np.where(moved[:, :, 0] >= 0, np.abs(ac.slot_terms(sc, s, moved)[0] - t), 0.0))
    plant("moved by a cell", e, q, **lc.with_slot(s, e, q, moved[e, q]))
    e, q = lc.best(size)
    plant("emptied", e, q, **lc.with_slot(s, e, q, None))
    # the tail lane; one weight
    lc.stands(sc, f"last Ex entry ({len(s.ijk) - 1}) dropped", lc.replace_list(spec, "aniso", n, **ac.without_last(s)), [(0, s.ijk[-1])])
    rel, _ = lc.resolved(sc, f"g[{e}, {q}] of Ex", lambda rel: lc.replace_list(spec, "aniso", n, **lc.scaled(s, "g", (e, q), rel)), [(0, s.ijk[e])])
    print(f"[plant] aniso: the measure resolves one weight g at rel {rel:g}")
