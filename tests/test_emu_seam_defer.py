"""Deferred seam repair (FDTD_OPT_SEAM_DEFER; seam_kernel's compact mode, the REP instantiations of fused2_step_kernel and
seam_flush_kernel, fdtd_kernels2.hpp) on the CPU emulator: a plain step pair that is followed by another plain pair leaves the
seven repaired values per seam row in a compact array the next sweep's edge lanes read.  The values are the ones seam_kernel
stores into the fields otherwise, so all six fields after N steps are the same bits with the option on, with it off and with
single steps — whatever lies on or next to a seam, and whatever interrupts the run of pairs."""
import numpy as np
import pytest

import tidy3d_amd.schema as td
from tidy3d_amd import lib as L
from tidy3d_amd.discretize import discretize
from tidy3d_amd.engine import HipEngine

from test_emu_fused2 import ABS, DL, MEDIA_WIDE, PEC, PMC_MIN, PMC_MIX, PULSE, _sim

TWO = (260, 9, 8)            # one seam, a four-cell last tile
THREE = (516, 6, 13)         # two seams, a short last tile
ONE = (32, 14, 10)           # no seam


ANY_W = 2                    # FDTD_OPT_SEAM_DEFER = 2: deferral at every workgroup size (-1 / 1, the default: sixteen-wave launches only)


def _run(spec, lib, twostep, defer, runs, probe=None, paged=-1):
    """-> fields, results, pairs, deferred pairs, flushes; probe(engine, run index) is called between the runs"""
    with HipEngine(spec, lib=lib, variant=L.VARIANT_FUSED, z_chunk=2) as e:
        e.set_option(L.OPT_ROWS, 3)
        e.set_option(L.OPT_TWOSTEP, twostep)
        e.set_option(L.OPT_SEAM_DEFER, defer)
        if paged >= 0:
            e.set_option(L.OPT_SRC_PAGED, paged)
        pairs = deferred = flushes = 0
        for q, r in enumerate(runs):
            st = e.run(r)
            ss = e.seam_stats()
            assert int(ss.seam_pending) == 0           # a run never returns with stale seam columns
            pairs += int(st.fused2_pairs)
            deferred += int(ss.seam_deferred_pairs)
            flushes += int(ss.seam_flushes)
            if probe:
                probe(e, q)
        return [e.get_field(c) for c in range(6)], e.results(), pairs, deferred, flushes


def _three_way(spec, lib, tw, runs, probe=None, defer=ANY_W, paged=-1):
    ref = _run(spec, lib, 0, 0, runs, probe, paged)
    off = _run(spec, lib, tw, 0, runs, probe, paged)
    on = _run(spec, lib, tw, defer, runs, probe, paged)
    assert ref[2] == 0 and off[2] == on[2] and off[3] == 0 and off[4] == 0
    assert max(float(np.abs(f).max()) for f in ref[0]) > 0
    for c in range(6):
        assert np.array_equal(off[0][c], ref[0][c]), c
        assert np.array_equal(on[0][c], ref[0][c]), c
    for k in ref[1]:
        assert np.array_equal(np.asarray(on[1][k]), np.asarray(off[1][k])), k
    return on


# (the sources of _sim on wide grids: dipoles ON column 255, between columns 256 and 257, next to both x walls)
@pytest.mark.parametrize("N,w,zc", [(TWO, 16, 32), (TWO, 4, 2), (TWO, 8, 3), (THREE, 5, 3), (THREE, 6, 32), (THREE, 16, 4)])
def test_vacuum_pairs_deferred_equal_single_steps(N, w, zc, emu_lib):
    """Runs of 11 and 15 steps (odd: 5 + 7 pairs and a single step each).  Every pair but the last of a run is followed by a plain
    pair: 4 + 6 deferred, nothing to flush."""
    disc = discretize(_sim(N, monitors=False), n_steps=26)
    disc.spec.decay_every = 0
    on = _three_way(disc.spec, emu_lib, w + 64 * zc, (11, 15))
    assert on[2] == 12 and on[3] == 4 + 6 and on[4] == 0, on[2:]


@pytest.mark.parametrize("N,w,zc", [(TWO, 6, 4), (THREE, 8, 5), (THREE, 16, 32)])
def test_materials_across_the_seam(N, w, zc, emu_lib):
    """A lossy bar through the seam at column 256, a sphere, a PEC box: the materials instantiation and its tile classes."""
    disc = discretize(_sim(N, monitors=False, structures=MEDIA_WIDE), n_steps=26)
    disc.spec.decay_every = 0
    assert len(disc.spec.media) > 2
    on = _three_way(disc.spec, emu_lib, w + 64 * zc, (11, 15))
    assert on[3] == 4 + 6 and on[4] == 0, on[2:]


@pytest.mark.parametrize("N,w,zc", [(TWO, 16, 32), (THREE, 6, 4)])
def test_absorber_layers(N, w, zc, emu_lib):
    """Absorber layers (damped in registers, in the seam kernel too, E^{n+2} included: the sweep applies the E-side sources of
    step n + 1 itself, so nothing follows the seam kernel): every pair but the last of a run is deferred."""
    disc = discretize(_sim(N, monitors=False, bspec=ABS), n_steps=26)
    disc.spec.decay_every = 0
    on = _three_way(disc.spec, emu_lib, w + 64 * zc, (11, 15))
    assert on[2] == 12 and on[3] == 4 + 6 and on[4] == 0, on[2:]


@pytest.mark.parametrize("N,w,zc,bspec", [(TWO, 16, 32, PMC_MIX), (THREE, 6, 4, PMC_MIN)])
def test_pmc_min_walls(N, w, zc, bspec, emu_lib):
    disc = discretize(_sim(N, monitors=False, structures=MEDIA_WIDE, bspec=bspec), n_steps=26)
    disc.spec.decay_every = 0
    on = _three_way(disc.spec, emu_lib, w + 64 * zc, (11, 15))
    assert on[3] == 4 + 6 and on[4] == 0, on[2:]


def test_monitors_over_the_seam_columns(emu_lib):
    """A DFT monitor over a whole plane and a time monitor (every 5 steps) around the seam columns 255 / 256: pairs that record, and
    pairs in front of a record, store into the fields as before; the records are the same bits."""
    N = TWO
    size = tuple(n * DL for n in N)
    mons = [td.FieldMonitor(center=(0, 0, 0), size=(td.inf, td.inf, 0), freqs=[3e14], name="f", interval_space=(1, 1, 1)),
            td.FieldTimeMonitor(center=(-0.5 * size[0] + 256 * DL, 0, 0), size=(6 * DL, 0.2, 0.2), name="t", interval=5, colocate=False)]
    disc = discretize(_sim(N, monitors=False).updated_copy(monitors=mons), n_steps=26)
    disc.spec.decay_every = 0
    on = _three_way(disc.spec, emu_lib, 16 + 64 * 32, (11, 15))
    assert on[4] == 0, on[2:]


def test_sparse_time_monitor_over_the_seam_columns(emu_lib):
    """A time monitor alone (every 5 steps) whose box holds the seam columns 255 / 256: the pairs between its records are deferred,
    the pairs that record (pair_record reads both sets) and the pairs in front of one (the look-ahead at rec_at(n + 2), rec_at(n + 3))
    are not — so nothing is ever flushed — and the records are the same bits."""
    N = TWO
    size = tuple(n * DL for n in N)
    mons = [td.FieldTimeMonitor(center=(-0.5 * size[0] + 256 * DL, 0, 0), size=(6 * DL, 0.2, 0.2), name="t", interval=5, colocate=False)]
    disc = discretize(_sim(N, monitors=False).updated_copy(monitors=mons), n_steps=41)
    disc.spec.decay_every = 0
    on = _three_way(disc.spec, emu_lib, 16 + 64 * 32, (41,))
    print("time monitor: pairs, deferred, flushes =", on[2:])
    assert on[2] > 0 and on[3] > 0 and on[3] < on[2] and on[4] == 0, on[2:]
    assert len(on[1]) > 0


def _cut_first_source(spec, n):
    sc = spec.sources[0]
    sc.wave_e, sc.wave_h = np.asarray(sc.wave_e)[:n].copy(), np.asarray(sc.wave_h)[:n].copy()


FLUSH_CASES = [(TWO, (), PEC), (THREE, (), PEC), (THREE, MEDIA_WIDE, PEC), (THREE, (), ABS), (TWO, MEDIA_WIDE, PEC)]


@pytest.mark.parametrize("N,structures,bspec", FLUSH_CASES)
def test_flush_in_front_of_a_pair_the_sweep_cannot_read_the_array_in(N, structures, bspec, emu_lib):
    """The first source list ends at step 10, the others go on: the pair of steps 8, 9 is deferred (the look-ahead sees no record,
    no decay check), the pair of steps 10, 11 carries paged source terms — not an instantiation that reads the repair array — and
    launch_fused2 flushes first.  Pairs 0 ... 4 deferred, ONE flush, none later (every later pair is a paged one)."""
    disc = discretize(_sim(N, monitors=False, structures=structures, bspec=bspec), n_steps=30)
    disc.spec.decay_every = 0
    _cut_first_source(disc.spec, 10)
    on = _three_way(disc.spec, emu_lib, 16 + 64 * 32, (30,), defer=1)
    assert on[2] == 15 and on[3] == 5 and on[4] == 1, on[2:]


@pytest.mark.parametrize("N,structures,bspec", FLUSH_CASES[:4])
def test_flush_in_front_of_a_single_step(N, structures, bspec, emu_lib):
    """The same with paged source terms switched off: while one list is spent and the others inject, steps are single steps — the
    run loop flushes in front of the first of them (step 10)."""
    disc = discretize(_sim(N, monitors=False, structures=structures, bspec=bspec), n_steps=30)
    disc.spec.decay_every = 0
    _cut_first_source(disc.spec, 10)
    on = _three_way(disc.spec, emu_lib, 16 + 64 * 32, (30,), defer=1, paged=0)
    assert on[2] == 5 and on[3] == 5 and on[4] == 1, on[2:]


def test_default_option_defers_sixteen_wave_launches_only(emu_lib):
    """-1 and 1 are the same setting: sixteen-wave launches defer, smaller workgroups (which would have to run the sixteen-wave
    instantiation) do not; 2 defers those too."""
    disc = discretize(_sim(TWO, monitors=False), n_steps=26)
    disc.spec.decay_every = 0
    for d in (-1, 1):
        assert _three_way(disc.spec, emu_lib, 16 + 64 * 32, (11, 15), defer=d)[3] == 4 + 6
        assert _three_way(disc.spec, emu_lib, 8 + 64 * 3, (11, 15), defer=d)[3] == 0
    assert _three_way(disc.spec, emu_lib, 8 + 64 * 3, (11, 15), defer=ANY_W)[3] == 4 + 6


def test_get_field_between_runs(emu_lib):
    """A run split into several fdtd_run calls with get_field (and set_field of what it returned) between them."""
    disc = discretize(_sim(THREE, monitors=False), n_steps=40)
    disc.spec.decay_every = 0
    seen = {}

    def probe(e, q):
        f = [e.get_field(c) for c in range(6)]
        seen.setdefault(q, []).append(f)
        if q == 1:
            e.set_field(2, f[2])

    on = _three_way(disc.spec, emu_lib, 8 + 64 * 5, (6, 9, 4, 8), probe)
    assert on[3] == 2 + 3 + 1 + 3 and on[4] == 0, on[2:]
    for q, runs in seen.items():            # (single steps, pairs, deferred pairs: the same fields at every stop)
        for c in range(6):
            assert np.array_equal(runs[1][c], runs[0][c]) and np.array_equal(runs[2][c], runs[0][c]), (q, c)


def test_decay_checks_interrupt_the_run_of_pairs(emu_lib):
    """A field-decay check every 6 steps reads the fields: the pair in front of it is not deferred."""
    disc = discretize(_sim(TWO, monitors=False), n_steps=26)
    disc.spec.decay_every = 6
    on = _three_way(disc.spec, emu_lib, 16 + 64 * 32, (26,))
    assert on[3] > 0 and on[4] == 0, on[2:]


@pytest.mark.parametrize("bspec", [td.BoundarySpec(x=td.Boundary.periodic(), y=td.Boundary(minus=td.PECBoundary(), plus=td.PECBoundary()),
                                                   z=td.Boundary(minus=td.PECBoundary(), plus=td.PECBoundary())),
                                   td.BoundarySpec(x=td.Boundary.pml(num_layers=4), y=td.Boundary(minus=td.PECBoundary(), plus=td.PECBoundary()),
                                                   z=td.Boundary.pml(num_layers=3))])
def test_clipped_sweeps_stay_undeferred(bspec, emu_lib):
    """Periodic x (the wrap is a seam of the clipped sweep) and a bulk clipped by CPML (shell pairs beside it read the columns next
    to the shell): their seam kernel stores into the fields, the option changes nothing."""
    disc = discretize(_sim(TWO, monitors=False, bspec=bspec), n_steps=26)
    disc.spec.decay_every = 0
    on = _three_way(disc.spec, emu_lib, 16 + 64 * 32, (11, 15))
    assert on[3] == 0 and on[4] == 0, on[2:]


def test_no_seam_no_deferral(emu_lib):
    disc = discretize(_sim(ONE, monitors=False), n_steps=26)
    disc.spec.decay_every = 0
    on = _three_way(disc.spec, emu_lib, 16 + 64 * 32, (11, 15))
    assert on[2] == 12 and on[3] == 0 and on[4] == 0, on[2:]


def test_option_switched_inside_one_engine(emu_lib):
    """The option switched inside one engine (A/B runs share one engine): a run with it on, one with it off, one with it on again —
    every run ends with nothing pending, and the fields are those of single steps."""
    disc = discretize(_sim(TWO, monitors=False), n_steps=30)
    disc.spec.decay_every = 0
    ref = _run(disc.spec, emu_lib, 0, 0, (10, 10, 10))
    with HipEngine(disc.spec, lib=emu_lib, variant=L.VARIANT_FUSED, z_chunk=2) as e:
        e.set_option(L.OPT_ROWS, 3)
        e.set_option(L.OPT_TWOSTEP, 16 + 64 * 32)
        counts = []
        for d in (1, 0, 1):
            e.set_option(L.OPT_SEAM_DEFER, d)
            e.run(10)
            counts.append(int(e.seam_stats().seam_deferred_pairs))
            assert int(e.seam_stats().seam_pending) == 0
        got = [e.get_field(c) for c in range(6)]
    assert counts == [4, 0, 4], counts
    for c in range(6):
        assert np.array_equal(got[c], ref[0][c]), c
