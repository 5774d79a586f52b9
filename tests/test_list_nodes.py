"""The whole-grid node lists held to their fp64 oracles node by node — the reference side (CPU; docs/history/LIST_NODES.md): what keeps
the measure of ``list_case.Scenario.check_nodes`` honest (excluded share, no listed node excluded), that the scenarios of each kind hold
a tail block, a list shorter than a wavefront, an empty and a wrapped slot, the planted deviations (clean fp64 oracle against an fp64
oracle whose spec has one list entry changed), and the neighbour tables built a second time from the convention in the kernel
headers, compared with the spec's entry by entry, after ``permute_spec``, and in the flat form the fdtd_add_* calls receive.  The engine
runs are in the kinds' own test_emu_* / test_gpu_* files (``check_scenario`` / ``check_run`` measure every run both ways)."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from tidy3d_amd.discretize import discretize
from tidy3d_amd.engine import HipEngine, permute_spec

import dense_state as ds
import list_case as lc
import modulation_case as mc
import nonlinear_case as nc
import pec_conformal_case as pc

KINDS = {"nonlinear": nc, "modulation": mc, "conformal": pc}
L2_BAR = 2e-5                 # the whole-array bar the plants are printed beside
FACTOR = 4.0                  # a plant stands at least this many bars high
RELS = (ds.REL, 1e-2, 1e-1)   # a coefficient plant steps up until it does; beyond 1e-1 the measure does not resolve the coefficient


# ---------------------------------------------------------------------------------------------------------------- inputs
@pytest.mark.parametrize("kind", list(KINDS))
def test_excluded_share_and_listed_nodes(kind):
    for label in KINDS[kind].Scenario.all_labels():
        sc = KINDS[kind].scenario(label)
        listed = sum(len(s.ijk) for s in sc.lists)
        print(f"[dense] {kind} {label} {sc.spec.shape}: excluded {100 * sc.share:.2f} % (cap {100 * lc.SHARE_CAP:.0f} %), {listed} listed nodes, none excluded")
        sc.check_inputs()


@pytest.mark.parametrize("kind", list(KINDS))
def test_scenarios_hold_tail_lanes_and_empty_and_wrapped_slots(kind):
    for what, found in lc.presence(KINDS[kind].Scenario).items():
        print(f"[dense] {kind}: {what}: " + (", ".join(f"{label} {comp} ({n})" for label, comp, n in found) or "none"))
        assert found, (kind, what)


@pytest.mark.parametrize("kind", list(KINDS))
def test_the_sentence_names_list_entry_and_slots(kind):
    sc = KINDS[kind].scenario("small_at_wall")
    s = sc.lists[0]
    n = len(s.ijk)
    said = sc.where(s.comp, s.ijk[n - 1])
    assert f"entry {n - 1} of {n} (block 0, lane {n - 1})" in said and "slots empty" in said and "wrapped" in said, said
    far = sc.where(s.comp, (0, 0, 0) if kind != "conformal" else (1, 1, 1))
    assert "not listed" in far and "cells (Chebyshev) from the nearest listed node" in far, far


# ---------------------------------------------------------------------------------------------------------------- planted deviations
def _stands(sc, name, spec, named, *how, under_l2=False):
    K, w, bar, l2, hit = lc.check_plant(sc, name, spec, named, *how)
    assert w.value >= FACTOR * bar, f"{sc.label} {name} K={K}: {w.value:.3e} is under {FACTOR:g} x the bar {bar:.3e}: {w}"
    assert hit, f"{sc.label} {name} K={K}: the worst node is not the planted one {named}: {w}"
    if under_l2:              # ... and the whole-array measure would have let it through
        assert l2 < L2_BAR, (sc.label, name, K, l2)
    return K, w, bar, l2


def _resolved(sc, name, make, named, *how):
    """the smallest rel of RELS at which the coefficient plant stands; the value is the measure's resolution for that coefficient"""
    for rel in RELS:
        K, w, bar, l2, hit = lc.check_plant(sc, f"{name} x (1 + {rel:g})", make(rel), named, *how)
        if w.value >= FACTOR * bar and hit:
            print(f"[plant] {sc.TAG} {sc.label} {name}: resolved at rel {rel:g}")
            return rel, l2
    raise AssertionError(f"{sc.label} {name}: not resolvable by the per-node measure up to rel {RELS[-1]:g}")


def _best(size):
    """(entry, slot) of the candidate at the median of the non-zero sizes: a node like most, chosen by the state alone — the largest
    candidate is also the one the whole-array figure sees best"""
    flat = np.flatnonzero(size.reshape(-1) > 0)
    assert flat.size
    pick = flat[np.argsort(size.reshape(-1)[flat], kind="stable")[flat.size // 2]]
    e, slot = np.unravel_index(int(pick), size.shape)
    return int(e), int(slot)


def test_planted_deviations_kerr():
    sc, n = nc.scenario("pec_box_blocks"), 0
    spec, s = sc.ref_spec(5), sc.lists[0]
    assert s.comp == 0
    for kind in ("moved", "emptied"):
        size, node = lc.slot_candidates(sc, s, kind)
        e, slot = _best(size)
        change = lc.with_slot(s, e, slot, node[e, slot] if kind == "moved" else None)
        _stands(sc, f"slot {slot} of Ex entry {e} {kind}", lc.replace_list(spec, "nonlinear", n, **change), [(0, s.ijk[e])], 5, under_l2=True)
    last = len(s.ijk) - 1
    zero = np.array(s.chi3)
    zero[last] = 0.0
    _stands(sc, "last Ex entry with chi3 = 0", lc.replace_list(spec, "nonlinear", n, chi3=zero), [(0, s.ijk[last])], 5)
    E = [np.asarray(f, np.float64) for f in sc.state[:3]]
    e = _best((np.abs(s.chi3) * nc.intensity(E, s) * np.abs(lc.value_at(E, 0, s.ijk)))[:, None])[0]
    rel, _ = _resolved(sc, f"chi3 of Ex entry {e}", lambda rel: lc.replace_list(spec, "nonlinear", n, **lc.scaled(s, "chi3", e, rel)), [(0, s.ijk[e])], 5)
    assert rel > ds.REL          # (the Kerr correction is a few percent of the field: 1e-3 of it is under the fp32 floor)
    # an empty slot at a wall filled with the node across it: the body against the x+ wall
    sc = nc.scenario("small_at_wall")
    spec, s = sc.ref_spec(5), sc.lists[0]
    size, node = lc.slot_candidates(sc, s, "filled")
    e, slot = _best(size)
    _stands(sc, f"empty slot {slot} of Ex entry {e} filled", lc.replace_list(spec, "nonlinear", 0, **lc.with_slot(s, e, slot, node[e, slot])),
            [(0, s.ijk[e])], 5)


def test_planted_deviations_modulation():
    sc, n = mc.scenario("pec_box_blocks"), 0
    spec, s = sc.ref_spec(), sc.lists[0]
    assert np.abs(s.d_eps).max() > 0
    last = len(s.ijk) - 1
    off = {name: np.array(getattr(s, name)) for name in ("d_eps", "d_sigma")}
    for a in off.values():
        a[last] = 0.0
    _stands(sc, f"last {ds.COMP[s.comp]} entry with d_eps = d_sigma = 0", lc.replace_list(spec, "modulation", n, **off), [(s.comp, s.ijk[last])])
    e = _best((np.abs(s.d_eps) * np.abs(lc.value_at(sc.state, s.comp, s.ijk)))[:, None])[0]
    _resolved(sc, f"d_eps of {ds.COMP[s.comp]} entry {e}", lambda rel: lc.replace_list(spec, "modulation", n, **lc.scaled(s, "d_eps", e, rel)),
              [(s.comp, s.ijk[e])])


def _face_and_edges(sc, cs, e):
    comps, nbr, _ = lc.conformal_slots(sc.spec, cs, unlisted_edges=False)
    return [(cs.comp, cs.ijk[e])] + [(comps[k], nbr[e, k]) for k in range(4) if nbr[e, k, 0] >= 0]


def _all_weights(sc, cs):
    """|double_weights| with no slot left out: what a unit E on each edge would add to the face, wall edges included"""
    return np.abs(pc.double_weights(sc.spec, dataclasses.replace(cs, nbr_ijk=np.zeros_like(cs.nbr_ijk))))


def test_planted_deviations_conformal():
    sc, n = pc.scenario("sphere_blocks"), 0
    spec, cs = sc.ref_spec(), sc.lists[0]
    assert cs.comp == 3
    for kind in ("moved", "emptied"):
        size, node = lc.slot_candidates(sc, cs, kind)
        e, slot = _best(size * _all_weights(sc, cs))
        change = lc.with_slot(cs, e, slot, node[e, slot] if kind == "moved" else None)
        _stands(sc, f"slot {slot} of Hx face {e} {kind}", lc.replace_list(spec, "conformal", n, **change), _face_and_edges(sc, cs, e))
    last = len(cs.ijk) - 1
    one = np.array(cs.l)
    one[last, :] = cs.area_eff[last]
    _stands(sc, "last Hx face with l / area_eff = 1", lc.replace_list(spec, "conformal", n, l=one), _face_and_edges(sc, cs, last))
    live = cs.nbr_ijk[:, :, 0] >= 0
    # what a relative change of l_k moves in the face's sum: (dt / mu0) (l_k / area_eff) / step_k times the edge's field in the state
    unit = _all_weights(sc, dataclasses.replace(cs, l=2.0 * np.repeat(cs.area_eff[:, None], 4, axis=1)))
    drive = np.where(live, unit * cs.l / cs.area_eff[:, None], 0.0)
    for k in range(4):
        j = np.where(live[:, k, None], cs.nbr_ijk[:, k], 0)
        drive[:, k] *= np.abs(lc.value_at(sc.state, cs.nbr_comp[k], j))
    e, k = _best(drive)
    rel, l2 = _resolved(sc, f"l_{k} of Hx face {e}", lambda rel: lc.replace_list(spec, "conformal", n, **lc.scaled(cs, "l", (e, k), rel)), _face_and_edges(sc, cs, e))
    assert rel == ds.REL and l2 < L2_BAR         # a weight 0.1 % off: seen node by node, let through by the whole-array bar
    e = _best(drive.sum(axis=1)[:, None])[0]
    _resolved(sc, f"area_eff of Hx face {e}", lambda rel: lc.replace_list(spec, "conformal", n, **lc.scaled(cs, "area_eff", e, rel)), _face_and_edges(sc, cs, e))
    # an empty slot at a wall filled with the node across it: the sphere through the x+ wall
    sc = pc.scenario("small_at_wall")
    spec = sc.ref_spec()
    best = None
    for n, cs in enumerate(sc.lists):
        size, node = lc.slot_candidates(sc, cs, "filled")
        size = size * _all_weights(sc, cs)
        if size.max() > 0 and best is None:
            best = (n, cs, *_best(size), node)
    n, cs, e, slot, node = best
    _stands(sc, f"empty slot {slot} of {ds.COMP[cs.comp]} face {e} filled", lc.replace_list(spec, "conformal", n, **lc.with_slot(cs, e, slot, node[e, slot])),
            _face_and_edges(sc, cs, e))


# ---------------------------------------------------------------------------------------------------------------- slots, a second time
def _aniso_specs():
    import test_aniso_bloch as tab
    out = {"fully_aniso_box": ds.case_spec("fully_aniso_box")}
    for name, sim in (("wrapped_cell", tab.wrapped_cell()), ("clear_case", tab.clear_case())):
        out[name] = discretize(sim, n_steps=2).spec
    return out


def _list_specs():
    """kind -> label -> spec, all four kinds"""
    out = {kind: {label: m.scenario(label).spec for label in m.Scenario.all_labels()} for kind, m in KINDS.items()}
    out["aniso"] = _aniso_specs()
    return out


def _compare(spec, attr, label):
    """the lists of ``attr`` on ``spec`` against the slots built here -> (slots compared, wrapped among them)"""
    slots = wrapped = 0
    for s in getattr(spec, attr):
        comps, nbr, wrap = lc.conformal_slots(spec, s) if attr == "conformal" else lc.kerr_slots(spec, s.comp, s.ijk)
        assert tuple(int(c) for c in s.nbr_comp) == tuple(comps), (label, attr, s.comp)
        assert s.nbr_ijk.shape == nbr.shape
        for e in range(len(s.ijk)):
            for q in range(nbr.shape[1]):
                assert tuple(s.nbr_ijk[e, q]) == tuple(nbr[e, q]), (label, attr, ds.COMP[s.comp], e, q, s.ijk[e], s.nbr_ijk[e, q], nbr[e, q])
        live = nbr[:, :, 0] >= 0
        if getattr(s, "nbr_wrap", None) is not None:         # the periods crossed, wherever the slot holds a node
            assert np.array_equal(np.asarray(s.nbr_wrap, np.int64)[live], wrap[live]), (label, attr, s.comp)
        # the wrap count a second way: a live slot whose node is not next to the listed one
        far = live & (np.abs(np.asarray(s.nbr_ijk) - s.ijk[:, None, :]) > 1).any(axis=2)
        big = np.asarray([n > 2 for n in spec.shape])          # (on an axis of two cells a wrapped node is also a next one)
        assert int(far.sum()) == int((live & ((wrap != 0) & big[None, None, :]).any(axis=2)).sum()), (label, attr, s.comp)
        slots, wrapped = slots + int(live.size), wrapped + int((wrap != 0).any(axis=2).sum())
    return slots, wrapped


@pytest.mark.parametrize("kind", ["nonlinear", "modulation", "conformal", "aniso"])
def test_the_neighbour_tables_built_a_second_time(kind):
    seen = {}
    for kind, specs in ((kind, _list_specs()[kind]),):
        for label, spec in specs.items():
            if kind == "modulation":                          # these lists carry no slots: nothing of a table can be wrong
                assert all(not hasattr(s, "nbr_ijk") for s in spec.modulation)
                continue
            seen[kind, label] = _compare(spec, kind, label)
            for shift in (1, 2):
                p = permute_spec(spec, shift)
                if kind == "aniso":                           # not renamed: the engine keeps the user's axes for them (below)
                    assert all(a is b for a, b in zip(p.aniso, spec.aniso))
                    continue
                assert [s.comp for s in getattr(p, kind)] == [(s.comp % 3 - shift) % 3 + 3 * (s.comp // 3) for s in getattr(spec, kind)]
                assert _compare(p, kind, f"{label} shift {shift}") == seen[kind, label]
            print(f"[slots] {kind} {label}: {seen[kind, label][0]} slots equal, {seen[kind, label][1]} of them wrapped; the same under both renamings")
    assert kind == "modulation" or any(w for _, w in seen.values()), kind          # wrapped slots among what was compared


def _recorded(lib, name, rows):
    """fdtd_add_<name> replaced by a function that keeps (component, cells [n], neighbour table [rows * n]) of every call and passes
    the call on -> (calls, restore)"""
    real, calls = getattr(lib.dll, name), []

    def keep(h, comp, n, cells, nbr, *rest):
        take = lambda p, m: np.ctypeslib.as_array((C.c_uint32 * m).from_address(p.value if hasattr(p, "value") else p)).copy()      # noqa: E731
        calls.append((int(comp), take(cells, n), take(nbr, rows * n)))
        return real(h, comp, n, cells, nbr, *rest)
    setattr(lib.dll, name, keep)
    return calls, lambda: setattr(lib.dll, name, real)


@pytest.mark.parametrize("kind,name,rows", [("nonlinear", "fdtd_add_nonlinear", 8), ("conformal", "fdtd_add_pec_conformal", 4), ("aniso", "fdtd_add_aniso", 8)])
def test_the_flat_tables_the_library_receives(kind, name, rows, emu_lib):
    """what ``HipEngine`` passes to fdtd_add_*: cell = (k ny + j) row + i with the device's row length, rows [slots][n] (the fully
    anisotropic lists: [n][slots], a slot of weight zero dropped), NO_NODE for an empty slot — under every renaming the engine takes"""
    checked = 0
    for label, spec in _list_specs()[kind].items():
        if spec.bloch is not None:
            continue                                          # (the Bloch layout moves every node by a ghost cell: tests/test_aniso_bloch.py)
        for shift in (0, 1, 2):
            calls, restore = _recorded(emu_lib, name, rows)
            try:
                with HipEngine(spec, lib=emu_lib, axis_shift=shift) as e:
                    dev, row, took = e.spec, e.nxp, e.axis_shift
            finally:
                restore()
            if kind == "aniso":
                assert took == 0                              # the coupling lists are laid out for the user's axes
            else:
                assert took == shift
            lists = getattr(dev, kind)
            assert [c for c, _, _ in calls] == [s.comp for s in lists if len(s.ijk)]
            for (comp, cells, nbr), s in zip(calls, [s for s in lists if len(s.ijk)]):
                n = len(s.ijk)
                mine = lc.conformal_slots(dev, s)[1] if kind == "conformal" else lc.kerr_slots(dev, s.comp, s.ijk)[1]
                want = lc.flat_table(dev.shape, row, mine)
                assert np.array_equal(cells, lc.flat_table(dev.shape, row, s.ijk[:, None, :])[0]), (label, shift, comp)
                if kind == "aniso":
                    got = nbr.reshape(n, rows).T
                    held = got != lc.NO_NODE
                    assert np.array_equal(got[held], want[held]) and not (held & (want == lc.NO_NODE)).any() and held.any(), (label, comp)
                else:
                    assert np.array_equal(nbr.reshape(rows, n), want), (label, shift, comp)
                checked += n
    assert checked > 0


def test_modulation_lists_keep_the_users_axes(emu_lib):
    spec = mc.scenario("small_at_wall").spec
    assert all(a is b for a, b in zip(permute_spec(spec, 1).modulation, spec.modulation))
    with HipEngine(spec, lib=emu_lib, axis_shift=1) as e:
        assert e.axis_shift == 0
