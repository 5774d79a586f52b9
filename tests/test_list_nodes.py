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
from tidy3d_amd.spec import BC_PERIODIC

import dense_state as ds
import list_case as lc
import modulation_case as mc
import nonlinear_case as nc
import pec_conformal_case as pc

KINDS = {"nonlinear": nc, "modulation": mc, "conformal": pc}


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
def test_planted_deviations_kerr():
    sc, n = nc.scenario("pec_box_blocks"), 0
    spec, s = sc.ref_spec(5), sc.lists[0]
    assert s.comp == 0
    for kind in ("moved", "emptied"):
        size, node = lc.slot_candidates(sc, s, kind)
        e, slot = lc.best(size)
        change = lc.with_slot(s, e, slot, node[e, slot] if kind == "moved" else None)
        lc.stands(sc, f"slot {slot} of Ex entry {e} {kind}", lc.replace_list(spec, "nonlinear", n, **change), [(0, s.ijk[e])], 5, under_l2=True)
    last = len(s.ijk) - 1
    zero = np.array(s.chi3)
    zero[last] = 0.0
    lc.stands(sc, "last Ex entry with chi3 = 0", lc.replace_list(spec, "nonlinear", n, chi3=zero), [(0, s.ijk[last])], 5)
    E = [np.asarray(f, np.float64) for f in sc.state[:3]]
    e = lc.best((np.abs(s.chi3) * nc.intensity(E, s) * np.abs(lc.value_at(E, 0, s.ijk)))[:, None])[0]
    rel, _ = lc.resolved(sc, f"chi3 of Ex entry {e}", lambda rel: lc.replace_list(spec, "nonlinear", n, **lc.scaled(s, "chi3", e, rel)), [(0, s.ijk[e])], 5)
    assert rel > ds.REL          # (the Kerr correction is a few percent of the field: 1e-3 of it is under the fp32 floor)
    # an empty slot at a wall filled with the node across it: the body against the x+ wall
    sc = nc.scenario("small_at_wall")
    spec, s = sc.ref_spec(5), sc.lists[0]
    size, node = lc.slot_candidates(sc, s, "filled")
    e, slot = lc.best(size)
    lc.stands(sc, f"empty slot {slot} of Ex entry {e} filled", lc.replace_list(spec, "nonlinear", 0, **lc.with_slot(s, e, slot, node[e, slot])),
            [(0, s.ijk[e])], 5)


def test_planted_deviations_modulation():
    sc, n = mc.scenario("pec_box_blocks"), 0
    spec, s = sc.ref_spec(), sc.lists[0]
    assert np.abs(s.d_eps).max() > 0
    last = len(s.ijk) - 1
    off = {name: np.array(getattr(s, name)) for name in ("d_eps", "d_sigma")}
    for a in off.values():
        a[last] = 0.0
    lc.stands(sc, f"last {ds.COMP[s.comp]} entry with d_eps = d_sigma = 0", lc.replace_list(spec, "modulation", n, **off), [(s.comp, s.ijk[last])])
    e = lc.best((np.abs(s.d_eps) * np.abs(lc.value_at(sc.state, s.comp, s.ijk)))[:, None])[0]
    lc.resolved(sc, f"d_eps of {ds.COMP[s.comp]} entry {e}", lambda rel: lc.replace_list(spec, "modulation", n, **lc.scaled(s, "d_eps", e, rel)),
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
        e, slot = lc.best(size * _all_weights(sc, cs))
        change = lc.with_slot(cs, e, slot, node[e, slot] if kind == "moved" else None)
        lc.stands(sc, f"slot {slot} of Hx face {e} {kind}", lc.replace_list(spec, "conformal", n, **change), _face_and_edges(sc, cs, e))
    last = len(cs.ijk) - 1
    one = np.array(cs.l)
    one[last, :] = cs.area_eff[last]
    lc.stands(sc, "last Hx face with l / area_eff = 1", lc.replace_list(spec, "conformal", n, l=one), _face_and_edges(sc, cs, last))
    live = cs.nbr_ijk[:, :, 0] >= 0
    # what a relative change of l_k moves in the face's sum: (dt / mu0) (l_k / area_eff) / step_k times the edge's field in the state
    unit = _all_weights(sc, dataclasses.replace(cs, l=2.0 * np.repeat(cs.area_eff[:, None], 4, axis=1)))
    drive = np.where(live, unit * cs.l / cs.area_eff[:, None], 0.0)
    for k in range(4):
        j = np.where(live[:, k, None], cs.nbr_ijk[:, k], 0)
        drive[:, k] *= np.abs(lc.value_at(sc.state, cs.nbr_comp[k], j))
    e, k = lc.best(drive)
    rel, l2 = lc.resolved(sc, f"l_{k} of Hx face {e}", lambda rel: lc.replace_list(spec, "conformal", n, **lc.scaled(cs, "l", (e, k), rel)), _face_and_edges(sc, cs, e))
    assert rel == ds.REL and l2 < lc.L2_BAR         # a weight 0.1 % off: seen node by node, let through by the whole-array bar
    e = lc.best(drive.sum(axis=1)[:, None])[0]
    lc.resolved(sc, f"area_eff of Hx face {e}", lambda rel: lc.replace_list(spec, "conformal", n, **lc.scaled(cs, "area_eff", e, rel)), _face_and_edges(sc, cs, e))
    # an empty slot at a wall filled with the node across it: the sphere through the x+ wall
    sc = pc.scenario("small_at_wall")
    spec = sc.ref_spec()
    best = None
    for n, cs in enumerate(sc.lists):
        size, node = lc.slot_candidates(sc, cs, "filled")
        size = size * _all_weights(sc, cs)
        if size.max() > 0 and best is None:
            best = (n, cs, *lc.best(size), node)
    n, cs, e, slot, node = best
    lc.stands(sc, f"empty slot {slot} of {ds.COMP[cs.comp]} face {e} filled", lc.replace_list(spec, "conformal", n, **lc.with_slot(cs, e, slot, node[e, slot])),
            _face_and_edges(sc, cs, e))


# ---------------------------------------------------------------------------------------------------------------- slots, a second time
def _aniso_specs():
    """``fully_aniso_box``, the clear Bloch cell of tests/test_aniso_bloch.py and the scenarios of tests/aniso_case.py (its
    ``bloch_xy_corner`` is ``wrapped_cell``)"""
    import aniso_case as ac
    import test_aniso_bloch as tab
    out = {"fully_aniso_box": ds.case_spec("fully_aniso_box"), "clear_case": discretize(tab.clear_case(), n_steps=2).spec}
    out.update({label: ac.scenario(label).spec for label in ac.Scenario.all_labels()})
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


def _recorded(lib, names, rows, more=()):
    """every fdtd_add_<name> of ``names`` replaced by a function that keeps (component, cells [n], neighbour table [rows * n], and per
    ctypes type of ``more`` the [rows * n] array of the argument that follows) of every call and passes the call on -> (calls, restore)"""
    real, calls = {name: getattr(lib.dll, name) for name in names}, []

    def take(p, m, t=C.c_uint32):
        return np.ctypeslib.as_array((t * m).from_address(p.value if hasattr(p, "value") else p)).copy()

    def keep(name):
        def call(h, comp, n, cells, nbr, *rest):
            calls.append((int(comp), take(cells, n), take(nbr, rows * n), *(take(p, rows * n, t) for p, t in zip(rest, more))))
            return real[name](h, comp, n, cells, nbr, *rest)
        return call
    for name in names:
        setattr(lib.dll, name, keep(name))
    return calls, lambda: [setattr(lib.dll, name, fn) for name, fn in real.items()]


def _aniso_layout(spec):
    """the device layout of the fully anisotropic lists from the spec alone -> (ghost cells in front of the real ones per axis, rows per
    plane, cells per row): one ghost cell at each end of an x / y axis with a Bloch phase (csrc/fdtd_run_bloch.hpp; walls for the kernels),
    rows padded to whole float4 unless x stays periodic"""
    nx, ny, _ = spec.shape
    ghost = [1 if a < 2 and spec.bloch is not None and spec.bloch[a] != 0.0 and spec.bc[a][0] == BC_PERIODIC and spec.shape[a] > 1 else 0 for a in range(3)]
    nx, ny = nx + 2 * ghost[0], ny + 2 * ghost[1]
    return np.asarray(ghost, np.int64), ny, nx if spec.bc[0][1] == BC_PERIODIC and not ghost[0] else nx + (-nx) % 4


def _check_aniso_call(where, spec, oracle, s, cells, nbr, w_new, w_old, wrap=None):
    """one fdtd_add_aniso / fdtd_add_aniso_bloch call against a second build made one node at a time from the geometry of the USER's
    grid (``lc.kerr_slots``: the raw neighbour index, the periods it left the cell by), moved by the ghost cells of the Bloch layout
    (``_aniso_layout``: nothing of it is read from the engine): cells, the [n][8] neighbours (a slot of weight zero dropped),
    w_new = (dt / eps0) g / Cb and w_old = w_new Ca with the FAR node's own Ca / Cb — the oracle's derivation, which agrees with the
    engine's to 1e-13: one fp32 ulp — and the wrap byte, codes 1 / 2 in bits 2a"""
    from oracle.fdtd_numpy import _EPS0
    n, (ghost, ny, row) = len(s.ijk), _aniso_layout(spec)
    _, mine, crossed = lc.kerr_slots(spec, s.comp, s.ijk)
    live = mine[:, :, 0] >= 0
    flat = lambda ijk: lc.flat_table((None, ny), row, np.where(ijk >= 0, ijk + ghost, -1))          # noqa: E731
    assert np.array_equal(cells, flat(s.ijk[:, None, :])[0]), where
    want_new = np.zeros((n, 8))
    want_old = np.zeros((n, 8))
    for slot in range(8):
        b, ok = s.nbr_comp[slot], live[:, slot]
        at = (mine[ok, slot, 2], mine[ok, slot, 1], mine[ok, slot, 0])
        ca, cb = (np.broadcast_to(t[b], spec.shape[::-1])[at] for t in (oracle.ca, oracle.cb))
        want_new[ok, slot] = np.where(cb == 0, 0.0, (spec.dt / _EPS0) * s.g[ok, slot] / np.where(cb == 0, 1.0, cb))
        want_old[ok, slot] = want_new[ok, slot] * ca
    got, held = nbr.reshape(n, 8), nbr.reshape(n, 8) != lc.NO_NODE
    assert np.array_equal(held, live & (want_new != 0)) and held.any(), where
    assert np.array_equal(got[held], flat(mine).T[held]), where
    for name, g32, want in (("w_new", w_new, want_new), ("w_old", w_old, want_old)):
        w32 = want.astype(np.float32)
        assert (np.abs(g32.reshape(n, 8) - w32)[held] <= np.spacing(np.abs(w32))[held]).all(), (where, name)
    if wrap is not None:
        code = ((crossed == 1) * 1 + (crossed == -1) * 2) @ np.array([1, 4, 16])
        assert np.array_equal(wrap.reshape(n, 8)[live], code[live]), where
    return int((crossed[held] != 0).any(axis=1).sum())


@pytest.mark.parametrize("kind,name,rows", [("nonlinear", "fdtd_add_nonlinear", 8), ("conformal", "fdtd_add_pec_conformal", 4), ("aniso", "fdtd_add_aniso", 8)])
def test_the_flat_tables_the_library_receives(kind, name, rows, emu_lib):
    """what ``HipEngine`` passes to fdtd_add_*: cell = (k ny + j) row + i with the device's row length, rows [slots][n], NO_NODE for an
    empty slot — under every renaming the engine takes.  The fully anisotropic lists (``_check_aniso_call``): fdtd_add_aniso and, under
    Bloch phases, fdtd_add_aniso_bloch on the ghost-cell layout, with their weights and wrap bytes; an engine asked for a renaming takes
    none and passes the same tables, periodic or Bloch"""
    from oracle.fdtd_numpy import OracleFdtd
    checked = across = 0
    names, more = ((name, name + "_bloch"), (C.c_float, C.c_float, C.c_uint8)) if kind == "aniso" else ((name,), ())
    for label, spec in _list_specs()[kind].items():
        if spec.bloch is not None and kind != "aniso":
            continue                                          # (the Bloch layout moves every node by a ghost cell)
        oracle = OracleFdtd(spec) if kind == "aniso" else None
        for shift in (0, 1, 2):
            calls, restore = _recorded(emu_lib, names, rows, more)
            try:
                with HipEngine(spec, lib=emu_lib, axis_shift=shift) as e:
                    dev, row, took = e.spec, e.nxp, e.axis_shift
            finally:
                restore()
            if kind == "aniso":
                assert took == 0, (label, shift)              # the coupling lists are laid out for the user's axes: no renaming is taken
                lists = list(spec.aniso) * (2 if spec.bloch is not None else 1)          # (the Re and the Im solver take the same lists)
                assert [c[0] for c in calls] == [s.comp for s in lists] and len(calls[0]) == (6 if spec.bloch is not None else 5)
                for call, s in zip(calls, lists):
                    across += _check_aniso_call((label, shift, ds.COMP[s.comp]), spec, oracle, s, *call[1:])
                    checked += len(s.ijk)
                continue
            assert took == shift
            lists = getattr(dev, kind)
            assert [c for c, _, _ in calls] == [s.comp for s in lists if len(s.ijk)]
            for (comp, cells, nbr), s in zip(calls, [s for s in lists if len(s.ijk)]):
                n = len(s.ijk)
                mine = lc.conformal_slots(dev, s)[1] if kind == "conformal" else lc.kerr_slots(dev, s.comp, s.ijk)[1]
                assert np.array_equal(cells, lc.flat_table(dev.shape, row, s.ijk[:, None, :])[0]), (label, shift, comp)
                assert np.array_equal(nbr.reshape(rows, n), lc.flat_table(dev.shape, row, mine)), (label, shift, comp)
                checked += n
    assert checked > 0 and (kind != "aniso" or across > 0)


def test_modulation_lists_keep_the_users_axes(emu_lib):
    spec = mc.scenario("small_at_wall").spec
    assert all(a is b for a, b in zip(permute_spec(spec, 1).modulation, spec.modulation))
    with HipEngine(spec, lib=emu_lib, axis_shift=1) as e:
        assert e.axis_shift == 0
