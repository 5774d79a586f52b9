"""Handles that CHANGE between runs, on the CPU emulator: lists and monitors added to a live handle, FDTD_OPT_* keys switched between
the runs of one engine (A / B / A), fdtd_reset, and get_field / set_field of all six fields in the middle of a run.  The first run of
a handle caches a lot (paged source tables, paged memory terms, tile classes, node tables, CPML parameter blocks, seam buffers, which
field / psi set is current); every scenario here holds the handle that changed afterwards to a FRESH handle — built from a spec that
holds the final configuration before its first run, advanced by single steps (FDTD_OPT_TWOSTEP = 0) — bit for bit, all six fields and
every monitor record, and one scenario per group to the fp64 oracle at the project's 2e-5 as well (handle and twin must not be wrong
together).  A list added at step k is in the fresh spec from the start with a waveform that is zero before step k.  Every scenario
prints its per-run counters and asserts from them that the changed handle took the path it claims to test."""
import copy
import ctypes as C
import dataclasses

import numpy as np
import pytest

import tidy3d_amd.schema as td
from tidy3d_amd import lib as L
from tidy3d_amd.discretize import discretize
from tidy3d_amd.engine import HipEngine, _cplx_f32, _f32, _ptr
from tidy3d_amd.exceptions import SolverLibraryError

import cases
import test_emu_disp as tdisp
import test_emu_shell2 as tsh2
import test_emu_srcpaged as tspg
from test_emu_fused2 import MEDIA, MEDIA_WIDE, _sim
from test_emu_seam_defer import ABS, THREE, TWO

ORACLE_BAR = 2e-5               # cases.run_case / tests/test_gpu_production_path.py
W16 = 16 + 64 * 32              # FDTD_OPT_TWOSTEP words: sixteen waves x 32 planes, and smaller workgroups
W5, W6, W8 = 5 + 64 * 3, 6 + 64 * 4, 8 + 64 * 5
ANY_W = 2                       # FDTD_OPT_SEAM_DEFER = 2: deferral at every workgroup size
OFF_DISABLED, OFF_SMALL, OFF_ADE, OFF_PMC_PLUS, OFF_SOURCES, OFF_VARIANT = 1, 2, 5, 7, 10, 11


# ---------------------------------------------------------------------------------------------------------------- the harness
def engine(spec, lib, opts=None, seed=None, **kw):
    e = HipEngine(spec, lib=lib, axis_shift=0, **({"variant": L.VARIANT_FUSED, "z_chunk": 2} | kw))
    for k, v in (opts or {}).items():
        e.set_option(k, v)
    if seed is not None:
        seed_fields(e, seed)
    return e


def seed_fields(e, seed):
    rng = np.random.default_rng(seed)
    for c in range(6):
        f = e.get_field(c)
        a = (1e-3 if c < 3 else 1e-3 / 376.73) * rng.uniform(-1, 1, size=f.shape)
        e.set_field(c, (a + 0j if np.iscomplexobj(f) else a).astype(f.dtype))


COUNTERS = ("fused2_pairs", "src_paged_pairs", "disp_pairs", "shell2_pairs", "fused2_off_reason", "graph_pairs", "two_step_pairs")


def counters(e, st):
    c = {k: int(getattr(st, k)) for k in COUNTERS}
    ss = e.seam_stats()
    assert int(ss.seam_pending) == 0
    c["seam_deferred_pairs"] = int(ss.seam_deferred_pairs)
    c["steps_done"] = int(st.steps_done)
    return c


def show(name, rows):
    for q, c in enumerate(rows):
        print(f"[lifecycle] {name}: run {q}: " + " ".join(f"{k}={v}" for k, v in c.items()))


def snapshot(e):
    return [e.get_field(c) for c in range(6)], e.results()


def fresh(spec, lib, n, seed=None, opts=None, **kw):
    """the reference: a handle complete before its first run, n single steps"""
    with engine(spec, lib, {L.OPT_TWOSTEP: 0} | (opts or {}), seed, **kw) as e:
        st = e.run(n)
        assert int(st.fused2_pairs) == 0 and int(st.two_step_pairs) == 0 and int(st.graph_pairs) == 0
        return snapshot(e) + (st,)


def same(ref, got):
    assert max(float(np.abs(f).max()) for f in ref[0]) > 0
    for c in range(6):
        assert np.array_equal(got[0][c], ref[0][c]), (c, float(np.abs(got[0][c] - ref[0][c]).max()), np.argwhere(got[0][c] != ref[0][c])[:4])
    assert set(got[1]) == set(ref[1])
    for k in ref[1]:
        assert np.array_equal(np.asarray(got[1][k]), np.asarray(ref[1][k])), k


def oracle_deviation(spec, got):
    """worst rel-L2 deviation from the fp64 oracle over the monitors and the final E / H triples: the norms of cases.run_case"""
    from oracle.fdtd_numpy import OracleFdtd
    o = OracleFdtd(spec)
    ref = o.run()
    worst = 0.0
    scale = max(np.linalg.norm(v) / np.sqrt(v.size) for v in ref.values()) if ref else 1.0
    for k in ref:
        den = max(np.linalg.norm(ref[k]), 0.5 * scale * np.sqrt(ref[k].size), 1e-300)
        worst = max(worst, float(np.linalg.norm(np.asarray(got[1][k]) - ref[k]) / den))
    en = np.sqrt(sum(np.linalg.norm(x) ** 2 for x in o.E))
    hn = np.sqrt(sum(np.linalg.norm(x) ** 2 for x in o.H))
    for c in range(3):
        worst = max(worst, float(np.linalg.norm(got[0][c] - o.E[c]) / en), float(np.linalg.norm(got[0][3 + c] - o.H[c]) / hn))
    return worst


def held_to_oracle(group, spec, got):
    dev = oracle_deviation(spec, got)
    print(f"[lifecycle] {group}: worst deviation from the fp64 oracle {dev:.3e} (bar {ORACLE_BAR:.0e})")
    assert dev <= ORACLE_BAR, dev


# ---- lists added to a live handle: the argument marshalling of HipEngine._setup (single slab, no axis renaming, no padding of x)
def add_point_list(e, s):
    assert e.axis_shift == 0 and e.pad_x == 0 and not any(e.ghost) and (e.z0, e.z1) == (0, e.spec.shape[2])
    nx, ny, _ = e.spec.shape
    ijk = np.asarray(s.ijk)
    for a in range(3):      # (an electric current on a PEC min wall, tangential to it, is dropped by _setup: the lists here keep off the walls)
        assert e.spec.bc[a][0] != 0 or not ((ijk[:, a] == 0) & (np.asarray(s.comp) < 3) & (np.asarray(s.comp) != a)).any()
    cell = (ijk[:, 2].astype(np.int64) * nx * ny + ijk[:, 1].astype(np.int64) * nx + ijk[:, 0]).astype(np.uint32)
    comp = np.ascontiguousarray(s.comp, dtype=np.int32)
    wre, wim, we, wh = _f32(s.w_re), _f32(s.w_im), _cplx_f32(s.wave_e), _cplx_f32(s.wave_h)
    e._chk(e.lib.dll.fdtd_add_point_source(e.handle, len(cell), _ptr(comp), _ptr(cell), _ptr(wre), _ptr(wim), len(s.wave_e), _ptr(we), _ptr(wh)),
           "fdtd_add_point_source")


def add_tfsf(e, t):
    assert e.axis_shift == 0 and e.pad_x == 0 and not any(e.ghost)
    nx, ny, _ = e.spec.shape

    def loc(ijk, *arrs):
        cell = (ijk[:, 2].astype(np.int64) * nx * ny + ijk[:, 1].astype(np.int64) * nx + ijk[:, 0]).astype(np.uint32)
        return [cell] + [np.ascontiguousarray(a) for a in arrs]
    ecell, ecomp, ew, eaux = loc(t.e_corr_ijk, t.e_corr_comp.astype(np.int32), t.e_corr_w.astype(np.float32), t.e_corr_aux.astype(np.int32))
    hcell, hcomp, hw, haux = loc(t.h_corr_ijk, t.h_corr_comp.astype(np.int32), t.h_corr_w.astype(np.float32), t.h_corr_aux.astype(np.int32))
    ae, be, ah, bh, wave = _f32(t.ae), _f32(t.be), _f32(t.ah), _f32(t.bh), _f32(t.wave)
    e._chk(e.lib.dll.fdtd_add_tfsf(e.handle, t.n_aux, _ptr(ae), _ptr(be), _ptr(ah), _ptr(bh), int(t.src_cell), len(wave), _ptr(wave),
                                   len(ecell), _ptr(ecomp), _ptr(ecell), _ptr(ew), _ptr(eaux),
                                   len(hcell), _ptr(hcomp), _ptr(hcell), _ptr(hw), _ptr(haux)), "fdtd_add_tfsf")


def add_monitor(e, m):
    assert e.axis_shift == 0 and not any(e.ghost)
    comps = np.asarray(m.comps, dtype=np.int32)
    lo, hi = np.asarray(m.lo, dtype=np.int32), np.asarray(m.hi, dtype=np.int32)
    steps = np.ascontiguousarray(m.steps, dtype=np.int64)
    if m.kind == "dft":
        pe, ph = _cplx_f32(m.phase_e), _cplx_f32(m.phase_h)
        mid = e.lib.dll.fdtd_add_monitor(e.handle, L.MON_DFT, len(comps), _ptr(comps), _ptr(lo), _ptr(hi), len(steps), _ptr(steps), len(m.freqs), _ptr(pe), _ptr(ph))
    else:
        mid = e.lib.dll.fdtd_add_monitor(e.handle, L.MON_TIME, len(comps), _ptr(comps), _ptr(lo), _ptr(hi), len(steps), _ptr(steps), 0, None, None)
    e._chk(mid, "fdtd_add_monitor")
    e.mon_ids.append((m, mid, (int(m.lo[2]), int(m.hi[2]))))


def burst(n_steps, k, amp=1.0):
    """a complex waveform that is zero before step k and strong right behind it"""
    n = np.arange(n_steps, dtype=np.float64)
    return np.where(n >= k, amp * np.exp(-((n - k - 7.0) / 4.0) ** 2) * np.exp(-0.35j * n), 0.0)


def late_list(s, k, n_steps, shift=(0, 0, 0)):
    """list s moved by `shift` cells, silent before step k"""
    w = burst(n_steps, k, float(np.abs(np.asarray(s.wave_e)).max()) * 3.0)
    return dataclasses.replace(s, ijk=(np.asarray(s.ijk) + np.asarray(shift)[None, :]).astype(np.int32), wave_e=w, wave_h=w.copy(), name="late")


def without(spec, sources=None, tfsf=None, monitors=None):
    sp = copy.copy(spec)
    if sources is not None:
        sp.sources = list(sources)
    if tfsf is not None:
        sp.tfsf = list(tfsf)
    if monitors is not None:
        sp.monitors = list(monitors)
    return sp


def segments(spec, lists):
    nx = spec.shape[0]
    assert nx % 4 == 0
    return {(int(k), int(j), int(i) // 256) for s in lists for i, j, k in np.asarray(s.ijk)}


def spec_of(sim, n_steps):
    disc = discretize(sim, n_steps=n_steps)
    disc.spec.decay_every = 0
    return disc.spec


def cut(s, n):
    return dataclasses.replace(s, wave_e=np.asarray(s.wave_e)[:n].copy(), wave_h=np.asarray(s.wave_h)[:n].copy())


# ------------------------------------------------------------------------------------------------- group 1: lists added between runs
@pytest.mark.parametrize("where", ["fresh_nodes", "segment_with_a_block"])
def test_point_list_added_after_a_run_that_paged(where, emu_lib):
    """Lists of different lengths (the first one ends at step 10): pairs 10 ... 13 of the first run carry paged source terms.  A list is
    added at step 14 — on row segments no list touched, or on one that holds a block already — and injects through the second run's eight
    pairs, all of them paged.  (Before spg_release: the new list had no slots, src_fill_points_kernel stored through a null pointer.)"""
    r1, r2 = 14, 16
    spec = spec_of(_sim(TWO, monitors=False), r1 + r2)
    spec.sources[0] = cut(spec.sources[0], 10)
    base = list(spec.sources)
    late = late_list(base[1], r1, r1 + r2, (2, 0, 0) if where == "segment_with_a_block" else (9, 3, 1))
    assert (segments(spec, [late]) <= segments(spec, base)) if where == "segment_with_a_block" else not (segments(spec, [late]) & segments(spec, base))
    assert not {tuple(r) for r in np.asarray(late.ijk)} & {tuple(r) for s in base for r in np.asarray(s.ijk)}
    spec.sources = base + [late]
    ref = fresh(spec, emu_lib, r1 + r2)
    with engine(without(spec, sources=base), emu_lib, {L.OPT_ROWS: 3, L.OPT_TWOSTEP: W16, L.OPT_SEAM_DEFER: 1}) as e:
        rows = [counters(e, e.run(r1))]
        add_point_list(e, late)
        rows.append(counters(e, e.run(r2)))
        got = snapshot(e)
    show(f"point list added after paging [{where}]", rows)
    assert rows[0]["fused2_pairs"] == 7 and rows[0]["src_paged_pairs"] == 2, rows
    assert rows[1]["fused2_pairs"] == 8 and rows[1]["src_paged_pairs"] == 8 and rows[1]["steps_done"] == r1 + r2, rows
    same(ref, got)
    if where == "fresh_nodes":
        held_to_oracle("group 1 (lists added between runs)", spec, got)


def _tfsf_spec(n_steps, dipoles=True, N=(40, 30, 28)):
    box = td.TFSF(center=(0, 0, 0), size=(1.0, 0.7, 0.6), source_time=tspg.PULSE, injection_axis=2, direction="+")
    dip = [td.PointDipole(center=(0.02, 0.01, 0.03), source_time=tspg.PULSE, polarization="Ey"),
           td.PointDipole(center=(-0.1, 0.05, -0.04), source_time=tspg.PULSE, polarization="Ez")] if dipoles else []
    return spec_of(tspg.sim(N, tspg.PEC, [box] + dip, [tspg.BALL], tspg.MON), n_steps)


def test_tfsf_box_added_after_a_run_with_point_lists_only(emu_lib):
    """The first run has two dipoles (node-table pairs; paging never tried).  A TFSF box is added at step 12: the second run's pairs carry
    its corrections as paged terms, the incident grid starts from rest as in the fresh handle (whose waveform is zero until then)."""
    r1, r2 = 12, 14
    spec = _tfsf_spec(r1 + r2)
    box = spec.tfsf[0]
    wave = np.asarray(box.wave, dtype=np.float64).copy()
    wave = np.where(np.arange(len(wave)) >= r1, np.real(burst(len(wave), r1, 3.0 * np.abs(wave).max())), 0.0)
    box = dataclasses.replace(box, wave=wave)
    spec.tfsf = [box]
    ref = fresh(spec, emu_lib, r1 + r2)
    with engine(without(spec, tfsf=[]), emu_lib, {L.OPT_ROWS: 3, L.OPT_TWOSTEP: W5}) as e:
        rows = [counters(e, e.run(r1))]
        add_tfsf(e, box)
        rows.append(counters(e, e.run(r2)))
        got = snapshot(e)
    show("TFSF box added after point lists", rows)
    assert rows[0]["fused2_pairs"] == 6 and rows[0]["src_paged_pairs"] == 0, rows
    assert rows[1]["fused2_pairs"] == 7 and rows[1]["src_paged_pairs"] == 7, rows
    same(ref, got)


def _late_box(spec, k):
    box = spec.tfsf[0]
    n = len(box.wave)
    wave = np.where(np.arange(n) >= k, np.real(burst(n, k, 3.0 * np.abs(np.asarray(box.wave)).max())), 0.0)
    return dataclasses.replace(box, wave=wave)


def test_tfsf_box_added_after_a_set_up_that_failed(emu_lib):
    """Lists of different lengths with FDTD_OPT_SRC_PAGED = 0: the first run's set-up gives up (state -1) and the steps behind step 10
    are single steps.  A TFSF box is added and the option switched on: the set-up is tried again for the lists of now and succeeds —
    the second run's pairs carry paged terms of the box and of the lists."""
    r1, r2 = 14, 14
    spec = _tfsf_spec(r1 + r2)
    spec.sources[0] = cut(spec.sources[0], 10)
    box = _late_box(spec, r1)
    spec.tfsf = [box]
    ref = fresh(spec, emu_lib, r1 + r2)
    with engine(without(spec, tfsf=[]), emu_lib, {L.OPT_ROWS: 3, L.OPT_TWOSTEP: W5, L.OPT_SRC_PAGED: 0}) as e:
        rows = [counters(e, e.run(r1))]
        add_tfsf(e, box)
        e.set_option(L.OPT_SRC_PAGED, 1)
        rows.append(counters(e, e.run(r2)))
        got = snapshot(e)
    show("TFSF box added after a failed set-up", rows)
    assert rows[0]["fused2_pairs"] == 5 and rows[0]["src_paged_pairs"] == 0, rows
    assert rows[1]["fused2_pairs"] == 7 and rows[1]["src_paged_pairs"] == 7, rows
    same(ref, got)


def test_point_list_added_after_a_tfsf_box_paged(emu_lib):
    """the run pages because of a TFSF box; a dipole list inside the box is added at step 12 and injects through paged pairs"""
    r1, r2 = 12, 14
    spec = _tfsf_spec(r1 + r2)
    late = late_list(spec.sources[0], r1, r1 + r2)
    spec.sources = [late]
    ref = fresh(spec, emu_lib, r1 + r2)
    with engine(without(spec, sources=[]), emu_lib, {L.OPT_ROWS: 3, L.OPT_TWOSTEP: W5}) as e:
        rows = [counters(e, e.run(r1))]
        add_point_list(e, late)
        rows.append(counters(e, e.run(r2)))
        got = snapshot(e)
    show("point list added after a TFSF box paged", rows)
    assert rows[0]["fused2_pairs"] == 6 and rows[0]["src_paged_pairs"] == 6, rows
    assert rows[1]["fused2_pairs"] == 7 and rows[1]["src_paged_pairs"] == 7, rows
    same(ref, got)


def test_point_list_added_to_a_handle_that_takes_paged_shell2_pairs(emu_lib):
    """CPML on all faces, a current sheet of hundreds of nodes through the layers (the reason the run pages), random initial fields:
    shell2 pairs whose boxes add paged terms.  A dipole list deep inside the bulk is added at step 12 — the boxes' cached flags and
    the tile classes are derived again from the new segment map."""
    r1, r2 = 12, 14
    N = (44, 30, 28)
    srcs = [td.UniformCurrentSource(center=(0, 0.23, 0), size=(td.inf, 0, td.inf), source_time=tspg.PULSE, polarization="Ez"),
            td.PointDipole(center=(0.02, 0.01, 0.03), source_time=tspg.PULSE, polarization="Ey")]
    spec = spec_of(tspg.sim(N, tspg.PML, srcs, [tspg.BALL], tspg.MON), r1 + r2)
    assert sum(len(s.comp) for s in spec.sources[:-1]) > 256
    base = spec.sources[:-1]
    late = late_list(spec.sources[-1], r1, r1 + r2, (4, -5, -3))
    assert not segments(spec, [late]) & segments(spec, base)
    spec.sources = base + [late]
    opts = {L.OPT_ROWS: 3, L.OPT_PML_SPLIT: 1, L.OPT_TWOSTEP: W5, L.OPT_SHELL_PAIRS: 1, L.OPT_SHELL2: 1}
    ref = fresh(spec, emu_lib, r1 + r2, seed=4)
    with engine(without(spec, sources=base), emu_lib, opts, seed=4) as e:
        rows = [counters(e, e.run(r1))]
        add_point_list(e, late)
        rows.append(counters(e, e.run(r2)))
        got = snapshot(e)
    show("point list added to paged shell2 pairs", rows)
    assert rows[0]["shell2_pairs"] == 6 and rows[0]["src_paged_pairs"] == 6, rows
    assert rows[1]["shell2_pairs"] == 7 and rows[1]["src_paged_pairs"] == 7, rows
    same(ref, got)


def test_handle_that_gave_up_paging_gains_nothing_from_a_new_list(emu_lib):
    """Three current sheets through one node would need a third layer: the first run gives paging up (state -1) and keeps single steps
    while the sheets inject.  A dipole list added afterwards has the set-up tried again — it gives up again: single steps, the same bits."""
    r1, r2 = 11, 15
    N = (40, 30, 28)
    three = [td.UniformCurrentSource(center=(0, 0.2, 0), size=(td.inf, 0, td.inf), source_time=tspg.PULSE, polarization="Ez"),
             td.UniformCurrentSource(center=(0.1, 0, 0), size=(0, td.inf, td.inf), source_time=tspg.PULSE, polarization="Ez"),
             td.UniformCurrentSource(center=(0, 0, 0.1), size=(td.inf, td.inf, 0), source_time=tspg.PULSE, polarization="Ez"),
             td.PointDipole(center=(-0.4, -0.3, -0.35), source_time=tspg.PULSE, polarization="Ex")]
    spec = spec_of(tspg.sim(N, tspg.PEC, three, [tspg.BALL]), r1 + r2)
    base = spec.sources[:-1]
    late = late_list(spec.sources[-1], r1, r1 + r2)
    spec.sources = base + [late]
    ref = fresh(spec, emu_lib, r1 + r2)
    with engine(without(spec, sources=base), emu_lib, {L.OPT_ROWS: 3, L.OPT_TWOSTEP: W5}) as e:
        rows = [counters(e, e.run(r1))]
        add_point_list(e, late)
        rows.append(counters(e, e.run(r2)))
        got = snapshot(e)
    show("gave up paging, list added", rows)
    for c in rows:      # (the one scenario that is single steps by design: the counters must say why)
        assert c["fused2_pairs"] == 0 and c["src_paged_pairs"] == 0 and c["fused2_off_reason"] == OFF_SOURCES, rows
    same(ref, got)


def test_point_list_added_to_a_handle_that_ran_without_sources(emu_lib):
    """Random initial fields, no list: plain (deferred) pairs.  Then a list: the node table is built, pairs inject from it."""
    r1, r2 = 12, 14
    spec = spec_of(_sim(TWO, monitors=False), r1 + r2)
    late = late_list(spec.sources[1], r1, r1 + r2)
    spec.sources = [late]
    ref = fresh(spec, emu_lib, r1 + r2, seed=3)
    with engine(without(spec, sources=[]), emu_lib, {L.OPT_ROWS: 3, L.OPT_TWOSTEP: W16, L.OPT_SEAM_DEFER: 1}, seed=3) as e:
        rows = [counters(e, e.run(r1))]
        add_point_list(e, late)
        rows.append(counters(e, e.run(r2)))
        got = snapshot(e)
    show("list added to a sourceless handle", rows)
    assert rows[0]["fused2_pairs"] == 6 and rows[0]["seam_deferred_pairs"] == 5, rows
    assert rows[1]["fused2_pairs"] == 7 and rows[1]["src_paged_pairs"] == 0 and rows[1]["seam_deferred_pairs"] == 6, rows
    same(ref, got)


def test_monitors_added_between_runs(emu_lib):
    """A time monitor (every 5 steps) and a DFT plane (every step) over the seam columns, added at step 12 with their first records at
    steps 15 and 13: the records equal the fresh handle's, and the second run takes the pairs a handle that knew them from the start takes."""
    r1, r2 = 12, 18
    size = tuple(n * 0.05 for n in TWO)
    mons = [td.FieldMonitor(center=(0, 0, 0), size=(td.inf, td.inf, 0), freqs=[3e14], name="f", interval_space=(1, 1, 1)),
            td.FieldTimeMonitor(center=(-0.5 * size[0] + 256 * 0.05, 0, 0), size=(6 * 0.05, 0.2, 0.2), name="t", interval=5, colocate=False)]
    spec = spec_of(_sim(TWO, monitors=False).updated_copy(monitors=mons), r1 + r2)
    late = []
    for m in spec.monitors:
        keep = np.asarray(m.steps) > r1
        assert keep.any() and not keep.all()
        late.append(dataclasses.replace(m, steps=np.asarray(m.steps)[keep], phase_e=None if m.phase_e is None else np.asarray(m.phase_e)[keep],
                                        phase_h=None if m.phase_h is None else np.asarray(m.phase_h)[keep]))
    spec.monitors = late
    opts = {L.OPT_ROWS: 3, L.OPT_TWOSTEP: W16, L.OPT_SEAM_DEFER: 1}
    ref = fresh(spec, emu_lib, r1 + r2)
    with engine(spec, emu_lib, opts) as e:          # (the monitors known from the start)
        known = [counters(e, e.run(r1)), counters(e, e.run(r2))]
    with engine(without(spec, monitors=[]), emu_lib, opts) as e:
        rows = [counters(e, e.run(r1))]
        for m in late:
            add_monitor(e, m)
        rows.append(counters(e, e.run(r2)))
        got = snapshot(e)
    show("monitors added between runs", rows)
    show("monitors known from the start", known)
    assert rows[0]["fused2_pairs"] == 6 and rows[1]["fused2_pairs"] > 0, rows
    assert {k: rows[1][k] for k in ("fused2_pairs", "seam_deferred_pairs")} == {k: known[1][k] for k in ("fused2_pairs", "seam_deferred_pairs")}
    assert all(float(np.abs(np.asarray(v)).max()) > 0 for v in ref[1].values())
    same(ref, got)


def _disp_spec(n_steps, N=tdisp.SHAPES["one_tile"], **kw):
    return spec_of(tdisp.sim_for(N, **kw), n_steps)


def test_add_ade_is_refused_once_the_memory_terms_are_paged(emu_lib):
    """fdtd_add_ade behind a run that paged the memory terms fails with its message; the handle goes on, the same bits as undisturbed."""
    r1, r2 = 11, 15
    spec = _disp_spec(r1 + r2)
    ref = fresh(spec, emu_lib, r1 + r2)
    with engine(spec, emu_lib, {L.OPT_ROWS: 3, L.OPT_TWOSTEP: W16}) as e:
        rows = [counters(e, e.run(r1))]
        idx = np.arange(4, dtype=np.uint32) + 40
        kap, bet = _cplx_f32(np.array([0.5 + 0.1j])), _cplx_f32(np.array([0.01 + 0.02j]))
        rc = e.lib.dll.fdtd_add_ade(e.handle, 0, idx.size, _ptr(idx), 1, _ptr(kap), _ptr(bet), C.c_float(0.1))
        assert rc != 0
        with pytest.raises(SolverLibraryError, match="paged already"):
            e._chk(rc, "fdtd_add_ade")
        rows.append(counters(e, e.run(r2)))
        got = snapshot(e)
    show("fdtd_add_ade refused", rows)
    assert rows[0]["disp_pairs"] == 5 and rows[1]["disp_pairs"] == 7 and rows[1]["fused2_pairs"] == 7, rows
    same(ref, got)


# --------------------------------------------------------------------------------------- group 2: options switched on a live handle
def switched(name, spec, lib, base, settings, r, seed=None, **kw):
    """one engine, one run of r steps per entry of `settings` (the options set in front of it) -> per-run counters; the result is held
    to the fresh single-step handle"""
    ref = fresh(spec, lib, r * len(settings), seed=seed, **kw)
    with engine(spec, lib, base, seed, **kw) as e:
        rows = []
        for opts in settings:
            for k, v in opts.items():
                e.set_option(k, v)
            rows.append(counters(e, e.run(r)))
        got = snapshot(e)
    show(name, rows)
    assert rows[-1]["steps_done"] == r * len(settings)
    same(ref, got)
    return rows, got


def test_src_paged_switched(emu_lib):
    """FDTD_OPT_SRC_PAGED 1 / 0 / 1 while a TFSF box injects: paged pairs, single steps (as in round 5), paged pairs again.  (Before
    spg_ok looked at the option the middle run paged too.)"""
    spec = _tfsf_spec(36, dipoles=False)
    rows, got = switched("SRC_PAGED 1/0/1", spec, emu_lib, {L.OPT_ROWS: 3, L.OPT_TWOSTEP: W5},
                         [{L.OPT_SRC_PAGED: 1}, {L.OPT_SRC_PAGED: 0}, {L.OPT_SRC_PAGED: 1}], 12)
    assert [c["src_paged_pairs"] for c in rows] == [6, 0, 6], rows
    assert [c["fused2_pairs"] for c in rows] == [6, 0, 6], rows
    held_to_oracle("group 2 (options switched)", spec, got)


def test_twostep_shapes_switched(emu_lib):
    """three x tiles with bodies: sixteen waves x 32 planes / single steps / six waves x 4 planes / the library's own choice (which, below 2^20
    cells, is single steps with FDTD_F2_OFF_TOO_SMALL)"""
    spec = spec_of(_sim(THREE, monitors=False, structures=MEDIA_WIDE), 40)
    rows, _ = switched("TWOSTEP shape/0/shape/-1", spec, emu_lib, {L.OPT_ROWS: 3, L.OPT_SEAM_DEFER: ANY_W},
                       [{L.OPT_TWOSTEP: W16}, {L.OPT_TWOSTEP: 0}, {L.OPT_TWOSTEP: W6}, {L.OPT_TWOSTEP: -1}], 10)
    assert [c["fused2_pairs"] for c in rows[:3]] == [5, 0, 5] and rows[1]["fused2_off_reason"] == OFF_DISABLED, rows
    # (-1: the library's own choice — on a grid of 2^15 cells it declines, and says so; the device module runs -1 where it takes pairs)
    assert rows[3]["fused2_pairs"] == 0 and rows[3]["fused2_off_reason"] == OFF_SMALL, rows


def _shell_spec(n_steps, N=tsh2.SHAPES["one_tile"]):
    mons = [td.FieldTimeMonitor(center=(0.03, 0.02, 0.01), size=(0, 0, 0), name="probe", interval=3, colocate=False)]
    return spec_of(tsh2._sim(N, tsh2.B_ALL, tsh2.MEDIA, mons), n_steps)


def test_shell_options_switched(emu_lib):
    """CPML on all faces, bodies through the layers, random initial fields; 10 steps = FIVE pairs per run, so the psi ping-pong ends on
    the other set each time.  Shell pairs by default / off (single steps) / on with another shape of the boxes and strips."""
    spec = _shell_spec(30)
    A = {L.OPT_SHELL_PAIRS: -1, L.OPT_SHELL2: 1, L.OPT_SHELL2_SHAPE: tsh2.shape_word(qw=9, ww=7), L.OPT_STRIP: 4 + 64 * 3}
    B = {L.OPT_SHELL_PAIRS: 0, L.OPT_SHELL2: 0}
    Cc = {L.OPT_SHELL_PAIRS: 2, L.OPT_SHELL2: 1, L.OPT_SHELL2_SHAPE: tsh2.shape_word(qw=16, ww=4, zcw=3, ws=2, zcs=5), L.OPT_STRIP: 8 + 64 * 4}
    rows, _ = switched("SHELL_PAIRS/SHELL2/SHELL2_SHAPE/STRIP", spec, emu_lib, {L.OPT_ROWS: 3, L.OPT_PML_SPLIT: 1, L.OPT_TWOSTEP: W5}, [A, B, Cc], 10, seed=7)
    assert [c["fused2_pairs"] for c in rows] == [5, 0, 5] and rows[1]["fused2_off_reason"] != 0, rows
    assert [c["shell2_pairs"] for c in rows] == [5, 0, 5], rows


def test_debug_sync_switched_on_shell2_pairs(emu_lib):
    spec = _shell_spec(30)
    base = {L.OPT_ROWS: 3, L.OPT_PML_SPLIT: 1, L.OPT_TWOSTEP: W5, L.OPT_SHELL_PAIRS: 1, L.OPT_SHELL2: 2}
    rows, _ = switched("DEBUG_SYNC 0/1/0", spec, emu_lib, base, [{L.OPT_DEBUG_SYNC: 0}, {L.OPT_DEBUG_SYNC: 1}, {L.OPT_DEBUG_SYNC: 0}], 10, seed=7)
    assert [c["shell2_pairs"] for c in rows] == [5, 5, 5], rows


def test_cpml_sweep_options_switched(emu_lib):
    """The single-step CPML sweeps (these keys act on them, so the handle takes single steps here): recursions inside the sweep on all
    axes / y and z / slab kernels, one launch / three, the z-chunk of the edge launches — psi written by one form is read by the next."""
    spec = _shell_spec(27, N=tsh2.SHAPES["two_x_tiles"])
    rows, _ = switched("PML_FUSED/PML_SPLIT/EDGE_ZCHUNK", spec, emu_lib, {L.OPT_ROWS: 3, L.OPT_TWOSTEP: 0},
                       [{L.OPT_PML_FUSED: 7, L.OPT_PML_SPLIT: 0, L.OPT_EDGE_ZCHUNK: -1}, {L.OPT_PML_FUSED: 6, L.OPT_PML_SPLIT: 1, L.OPT_EDGE_ZCHUNK: 2},
                        {L.OPT_PML_FUSED: 0, L.OPT_PML_SPLIT: 0, L.OPT_EDGE_ZCHUNK: 0}], 9, seed=5)
    assert all(c["fused2_off_reason"] == OFF_DISABLED for c in rows), rows


def test_tile_options_switched(emu_lib):
    """bodies in a few tiles of a two-tile grid: tile classes on / off / on, the tile orders, z-chunk and rows of the launches"""
    spec = spec_of(_sim(TWO, monitors=False, structures=MEDIA_WIDE), 40)
    rows, _ = switched("TILE_SPLIT/XCD_REMAP/ZCHUNK/ROWS", spec, emu_lib, {L.OPT_TWOSTEP: W8, L.OPT_SEAM_DEFER: ANY_W},
                       [{L.OPT_TILE_SPLIT: 1, L.OPT_XCD_REMAP: -1, L.OPT_ZCHUNK: 2, L.OPT_ROWS: 3}, {L.OPT_TILE_SPLIT: 0, L.OPT_XCD_REMAP: 0, L.OPT_ZCHUNK: 3, L.OPT_ROWS: 4},
                        {L.OPT_TILE_SPLIT: 1, L.OPT_XCD_REMAP: 1, L.OPT_ZCHUNK: 2, L.OPT_ROWS: 3}, {L.OPT_TILE_SPLIT: -1, L.OPT_XCD_REMAP: 5, L.OPT_ZCHUNK: 4, L.OPT_ROWS: 2}], 10)
    assert [c["fused2_pairs"] for c in rows] == [5, 5, 5, 5], rows


def test_variant_switched_over_paged_memory_terms(emu_lib):
    """dispersive bodies whose memory terms the first run paged: the two-pass kernels' ADE launch keeps them, the pairs of the third
    run read what it left"""
    spec = _disp_spec(33)
    rows, _ = switched("VARIANT fused/two-pass/fused", spec, emu_lib, {L.OPT_ROWS: 3, L.OPT_TWOSTEP: W16},
                       [{L.OPT_VARIANT: L.VARIANT_FUSED}, {L.OPT_VARIANT: L.VARIANT_ZMARCH}, {L.OPT_VARIANT: L.VARIANT_FUSED}], 11)
    assert [c["disp_pairs"] for c in rows] == [5, 0, 5] and rows[1]["fused2_off_reason"] == OFF_VARIANT, rows


def test_tblock_switched(emu_lib):
    """the slab-interleaved two-step schedule (eight planes per slab) between runs of plain pairs"""
    spec = spec_of(_sim((32, 14, 16), monitors=False, structures=MEDIA), 30)
    rows, _ = switched("TBLOCK 0/8/0", spec, emu_lib, {L.OPT_ROWS: 3, L.OPT_TWOSTEP: W5}, [{L.OPT_TBLOCK: 0}, {L.OPT_TBLOCK: 8}, {L.OPT_TBLOCK: 0}], 10)
    assert [c["two_step_pairs"] > 0 for c in rows] == [False, True, False], rows
    assert [c["fused2_pairs"] for c in rows] == [5, 0, 5], rows


def test_disp_cannot_be_switched_off_once_paged(emu_lib):
    """FDTD_OPT_DISP = 0 behind a run that paged the memory terms: refused as documented, nothing changes, the run goes on"""
    r1, r2 = 11, 15
    spec = _disp_spec(r1 + r2)
    ref = fresh(spec, emu_lib, r1 + r2)
    with engine(spec, emu_lib, {L.OPT_ROWS: 3, L.OPT_TWOSTEP: W16}) as e:
        rows = [counters(e, e.run(r1))]
        with pytest.raises(SolverLibraryError, match="bad key/value"):
            e.set_option(L.OPT_DISP, 0)
        rows.append(counters(e, e.run(r2)))
        got = snapshot(e)
    show("DISP = 0 after paging", rows)
    assert [c["disp_pairs"] for c in rows] == [5, 7], rows
    same(ref, got)


# ------------------------------------------------------------------------------------------- group 3: fdtd_reset = a fresh handle
def after_reset(name, spec, lib, opts, k, n, seed=None, proof=None, **kw):
    """k steps, reset (random initial fields set again), n steps — against a fresh handle's n single steps: fields, records, steps_done,
    field_decay, stopped_early (and with them the step at which a shutoff stops)"""
    ref = fresh(spec, lib, n, seed=seed, **kw)
    with engine(spec, lib, opts, seed, **kw) as e:
        rows = [counters(e, e.run(k))]
        first = e.stats()
        e.reset()
        assert int(e.stats().steps_done) == 0
        if seed is not None:
            seed_fields(e, seed)
        st = e.run(n)
        rows.append(counters(e, st))
        got = snapshot(e)
    show(name, rows)
    if proof:
        proof(rows)
    same(ref, got)
    for key in ("steps_done", "stopped_early", "field_decay", "diverged"):
        assert getattr(st, key) == getattr(ref[2], key), (key, getattr(st, key), getattr(ref[2], key))
    return rows, first, st, got


def pairs_in_both(key="fused2_pairs"):
    def proof(rows):
        assert rows[0][key] > 0 and rows[1][key] > 0, rows
    return proof


def test_reset_after_shell2_pairs(emu_lib):
    """CPML psi after an odd number of pairs (both sides on their other sets), monitors, random initial fields"""
    spec = _shell_spec(16)
    opts = {L.OPT_ROWS: 3, L.OPT_PML_SPLIT: 1, L.OPT_TWOSTEP: W5, L.OPT_SHELL_PAIRS: 1, L.OPT_SHELL2: 1}
    rows, *_ = after_reset("reset: shell2 pairs", spec, emu_lib, opts, 10, 16, seed=7, proof=pairs_in_both("shell2_pairs"))
    assert rows[0]["shell2_pairs"] == 5


def test_reset_after_paged_dispersive_pairs(emu_lib):
    spec = _disp_spec(16, monitors=[td.FieldTimeMonitor(center=(0.02, 0.01, 0.03), size=(0, 0, 0), name="p", interval=1, colocate=False)])
    _, _, _, got = after_reset("reset: paged dispersive cells", spec, emu_lib, {L.OPT_ROWS: 3, L.OPT_TWOSTEP: W16}, 11, 16, proof=pairs_in_both("disp_pairs"))
    held_to_oracle("group 3 (fdtd_reset)", spec, got)


def test_reset_after_tfsf_box_and_paged_source_terms(emu_lib):
    """the incident grid and the paged source arrays of the last pair are left behind; DFT and time monitors"""
    spec = _tfsf_spec(16)
    after_reset("reset: TFSF box, paged source terms", spec, emu_lib, {L.OPT_ROWS: 3, L.OPT_TWOSTEP: W5}, 14, 16, proof=pairs_in_both("src_paged_pairs"))


def test_reset_after_deferred_seam_pairs_in_absorber_layers(emu_lib):
    spec = spec_of(_sim(TWO, monitors=False, bspec=ABS), 16)
    rows, *_ = after_reset("reset: absorber layers, deferred seam pairs", spec, emu_lib, {L.OPT_ROWS: 3, L.OPT_TWOSTEP: W16, L.OPT_SEAM_DEFER: 1}, 13, 16,
                           proof=pairs_in_both())
    assert rows[0]["seam_deferred_pairs"] > 0, rows


def test_reset_after_a_decay_check_stopped_the_run(emu_lib):
    """Random fields between absorber layers only decay: the check stops the first run early.  After the reset energy_max starts
    over — the second run stops at the step a fresh handle stops at."""
    spec = spec_of(_sim(TWO, monitors=False, bspec=ABS), 60)
    spec.sources = []
    spec.decay_every, spec.shutoff, spec.decay_ref_step = 4, 0.93, 0
    rows, first, st, _ = after_reset("reset: stopped early", spec, emu_lib, {L.OPT_ROWS: 3, L.OPT_TWOSTEP: W16}, 60, 60, seed=11)
    print(f"[lifecycle] reset: stopped early: first run stopped at step {int(first.steps_done)}, after the reset at {int(st.steps_done)}")
    assert int(first.stopped_early) == 1 and int(st.stopped_early) == 1 and 0 < int(st.steps_done) < 60
    assert int(first.steps_done) == int(st.steps_done) and first.field_decay == st.field_decay


def single_steps(*reasons):
    """a workload that keeps single steps by design: the counters must name one of the reasons it has for that"""
    def proof(rows):
        assert all(c["fused2_pairs"] == 0 and c["two_step_pairs"] == 0 and c["fused2_off_reason"] in reasons for c in rows), rows
    return proof


pmc_plus_proof = single_steps(OFF_SMALL, OFF_PMC_PLUS)      # (at this size the first reason named is the grid's)


def test_reset_with_pmc_plus_faces(emu_lib):
    spec = spec_of(cases.pmc_plus_mix(), 30)
    after_reset("reset: pmc_plus_mix", spec, emu_lib, {}, 17, 30, proof=pmc_plus_proof)


def test_reset_with_a_fully_anisotropic_body(emu_lib):
    spec = spec_of(cases.fully_aniso_box(), 30)
    after_reset("reset: fully anisotropic body", spec, emu_lib, {}, 17, 30, proof=single_steps(OFF_SMALL, OFF_ADE), variant=L.VARIANT_AUTO, z_chunk=0)


def _bloch_run(name, spec, lib, runs, reset_after=None, opts=None):
    with HipEngine(spec, lib=lib) as e:
        assert e.twin is not None
        for k, v in (opts or {}).items():
            e.set_option(k, v)
            e.twin.set_option(k, v)
        rows = []
        for q, r in enumerate(runs):
            st = e.run(r)
            rows.append(counters(e, st))
            if reset_after == q:
                e.reset()
                assert int(e.stats().steps_done) == 0 and int(e.twin.stats().steps_done) == 0
        show(name, rows)
        return snapshot(e), st, e.twin.stats(), rows


@pytest.mark.parametrize("aniso", [False, True])
def test_reset_of_a_bloch_pair(aniso, emu_lib):
    """the twin handle (imaginary part) is reset with the handle; with and without fully anisotropic coupling lists.  fdtd_run_bloch
    advances the pair by single steps only (no pair path: fused2_off_reason stays 0 on it), which the counters must show."""
    if aniso:
        from test_aniso_bloch import clear_case
        sim = clear_case()
    else:
        sim = cases.bloch_box()
    spec = spec_of(sim, 24)
    ref, st0, tw0, rows0 = _bloch_run(f"reset: Bloch pair (aniso={aniso}), fresh", spec, emu_lib, (24,), opts={L.OPT_TWOSTEP: 0})
    got, st1, tw1, rows1 = _bloch_run(f"reset: Bloch pair (aniso={aniso})", spec, emu_lib, (13, 24), reset_after=0)
    for c in rows0 + rows1:
        assert c["fused2_pairs"] == 0 and c["two_step_pairs"] == 0 and c["graph_pairs"] == 0 and c["src_paged_pairs"] == 0, (rows0, rows1)
    for a, b in ((st0, st1), (tw0, tw1)):
        for key in ("steps_done", "stopped_early", "field_decay", "diverged"):
            assert getattr(a, key) == getattr(b, key), (key, getattr(a, key), getattr(b, key))
    assert int(st1.steps_done) == 24
    same(ref, got)


# ------------------------------------------------------------------------------ group 4: get_field / set_field on stateful handles
def round_trip(name, spec, lib, opts, k, n, seed=None, proof=None, **kw):
    """k steps, get_field of all six, set_field of exactly those arrays, the remaining n - k steps: the uninterrupted run"""
    ref = fresh(spec, lib, n, seed=seed, **kw)
    with engine(spec, lib, opts, seed, **kw) as e:
        rows = [counters(e, e.run(k))]
        f = [e.get_field(c) for c in range(6)]
        for c in range(6):
            e.set_field(c, f[c])
        for c in range(6):
            assert np.array_equal(e.get_field(c), f[c]), c
        rows.append(counters(e, e.run(n - k)))
        got = snapshot(e)
    show(name, rows)
    if proof:
        proof(rows)
    same(ref, got)
    return got


def test_round_trip_with_paged_dispersive_cells(emu_lib):
    """the ADE e_old gather of fdtd_set_field against pole states and paged memory terms in mid-run"""
    spec = _disp_spec(26)
    got = round_trip("round trip: paged dispersive cells", spec, emu_lib, {L.OPT_ROWS: 3, L.OPT_TWOSTEP: W16}, 11, 26, proof=pairs_in_both("disp_pairs"))
    held_to_oracle("group 4 (get_field / set_field)", spec, got)


def test_round_trip_with_shell2_pairs(emu_lib):
    spec = _shell_spec(26)
    opts = {L.OPT_ROWS: 3, L.OPT_PML_SPLIT: 1, L.OPT_TWOSTEP: W5, L.OPT_SHELL_PAIRS: 1, L.OPT_SHELL2: 1}
    round_trip("round trip: shell2 / CPML", spec, emu_lib, opts, 10, 26, seed=7, proof=pairs_in_both("shell2_pairs"))


def test_round_trip_with_periodic_z(emu_lib):
    """the ghost planes fdtd_set_field refills (periodic z: shell pairs with the planes next to the faces in the shell)"""
    bspec = td.BoundarySpec(x=td.Boundary(minus=td.PECBoundary(), plus=td.PECBoundary()), y=td.Boundary(minus=td.PMCBoundary(), plus=td.PECBoundary()),
                            z=td.Boundary.periodic())
    spec = spec_of(_sim((36, 14, 12), monitors=True, structures=MEDIA, bspec=bspec), 26)
    round_trip("round trip: periodic z", spec, emu_lib, {L.OPT_ROWS: 3, L.OPT_TWOSTEP: W5, L.OPT_SHELL_PAIRS: 1}, 11, 26, proof=pairs_in_both())


def test_round_trip_with_pmc_plus_faces(emu_lib):
    spec = spec_of(cases.pmc_plus_mix(), 30)
    round_trip("round trip: pmc_plus_mix", spec, emu_lib, {}, 13, 30, proof=pmc_plus_proof)
