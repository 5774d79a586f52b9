"""Handles that change between runs, on the device: a handful of the scenarios of tests/test_emu_lifecycle.py (which has the cases
proper, and the harness) at shapes the emulator does not reach — three x tiles with sixteen-wave launches, the bench workloads at
256^3 — and the options the emulator compiles away (FDTD_OPT_MEM_HINTS, FDTD_OPT_GRAPH).  The reference is the same: a fresh handle,
complete before its first run, advanced by single steps; all six fields and every record bit for bit, one scenario against the fp64
oracle at 2e-5, the path taken asserted from the per-run counters."""
import pytest

import tidy3d_amd.schema as td
from tidy3d_amd import lib as L

import cases
import test_emu_lifecycle as lc
from cases import DL, PULSE
from test_gpu_seam_defer import BAR, N, _sim

pytestmark = pytest.mark.gpu

W16 = lc.W16
DEV = {L.OPT_PLACEMENT_TRIES: 0}


def test_point_list_added_after_a_run_that_paged(hip_lib):
    """three x tiles, bodies through a seam; the first list ends at step 10 (paged pairs from there on), a list is added at step 20 on
    row segments no list touched and injects through the second run's paged pairs"""
    r1, r2 = 20, 30
    spec = lc.spec_of(_sim(structures=BAR), r1 + r2)
    spec.sources[0] = lc.cut(spec.sources[0], 10)
    base = list(spec.sources)
    late = lc.late_list(base[3], r1, r1 + r2, (40, 9, -7))
    assert not (lc.segments(spec, [late]) & lc.segments(spec, base))
    spec.sources = base + [late]
    ref = lc.fresh(spec, hip_lib, r1 + r2, opts=DEV, z_chunk=0)
    with lc.engine(lc.without(spec, sources=base), hip_lib, DEV | {L.OPT_TWOSTEP: W16}, z_chunk=0) as e:
        rows = [lc.counters(e, e.run(r1))]
        lc.add_point_list(e, late)
        rows.append(lc.counters(e, e.run(r2)))
        got = lc.snapshot(e)
    lc.show("device: point list added after paging", rows)
    assert rows[0]["fused2_pairs"] == 10 and rows[0]["src_paged_pairs"] == 5, rows
    assert rows[1]["fused2_pairs"] == 15 and rows[1]["src_paged_pairs"] == 15, rows
    lc.same(ref, got)


def _tfsf_spec(n_steps):
    sx = N[0] * DL
    box = td.TFSF(center=(-0.5 * sx + 256 * DL, 0, 0), size=(3.0, 2.4, 1.8), source_time=PULSE, injection_axis=2, direction="+")
    ball = td.Structure(geometry=td.Sphere(center=(box.center[0] + 0.05, 0, 0), radius=0.6), medium=td.Medium(permittivity=2.5))
    mons = [td.FieldMonitor(center=(0, 0, 0), size=(td.inf, td.inf, 0), freqs=[3e14], name="f", colocate=False)]
    sim = _sim(structures=[ball]).updated_copy(sources=[box], monitors=mons)
    return lc.spec_of(sim, n_steps)


def test_src_paged_switched(hip_lib):
    """a TFSF box over the seam at column 256 injecting: paged pairs / single steps / paged pairs inside one engine"""
    spec = _tfsf_spec(60)
    rows, _ = lc.switched("device: SRC_PAGED 1/0/1", spec, hip_lib, DEV | {L.OPT_TWOSTEP: W16},
                          [{L.OPT_SRC_PAGED: 1}, {L.OPT_SRC_PAGED: 0}, {L.OPT_SRC_PAGED: 1}], 20, z_chunk=0)
    assert [c["src_paged_pairs"] for c in rows] == [10, 0, 10] and [c["fused2_pairs"] for c in rows] == [10, 0, 10], rows


def _bench_spec(workload, n_steps, n=256):
    from bench import build_spec
    return build_spec(n, n_steps, workload)


def test_mem_hints_switched_on_bench_v0(hip_lib):
    """non-temporal field stores on / off / on (device only): sixteen-wave plain pairs of the 256^3 vacuum workload"""
    spec = _bench_spec("v0", 60)
    rows, _ = lc.switched("device: MEM_HINTS 1/0/1 (v0 256^3)", spec, hip_lib, DEV, [{L.OPT_MEM_HINTS: 1}, {L.OPT_MEM_HINTS: 0}, {L.OPT_MEM_HINTS: 1}], 20,
                          seed=1, z_chunk=0)
    assert all(c["fused2_pairs"] > 0 for c in rows), rows


def test_graphs_do_not_outlive_a_change_of_tile_shape_and_sources(hip_lib):
    """captured step pairs off / on / off / on on the 256^3 CPML workload (single-step sweeps: the graphs hold them), with the tile
    shape changed and a source list added between the two captured runs"""
    r = 20
    spec = _bench_spec("v2", 4 * r)
    late = lc.late_list(spec.sources[0], 3 * r, 4 * r, (11, -9, 5))
    ref_spec = lc.without(spec, sources=list(spec.sources) + [late])
    ref = lc.fresh(ref_spec, hip_lib, 4 * r, seed=2, opts=DEV, z_chunk=0)
    with lc.engine(spec, hip_lib, DEV | {L.OPT_TWOSTEP: 0, L.OPT_PML_SPLIT: 0}, seed=2, z_chunk=0) as e:
        rows = []
        for q, g in enumerate((0, 1, 0, 1)):
            e.set_option(L.OPT_GRAPH, g)
            if q == 3:
                e.set_option(L.OPT_ZCHUNK, 8)
                e.set_option(L.OPT_ROWS, 4)
                lc.add_point_list(e, late)
            rows.append(lc.counters(e, e.run(r)))
        got = lc.snapshot(e)
    lc.show("device: GRAPH 0/1/0/1 (v2 256^3)", rows)
    assert [c["graph_pairs"] > 0 for c in rows] == [False, True, False, True], rows
    lc.same(ref, got)


def test_shell_options_switched_over_three_x_tiles(hip_lib):
    """CPML on all faces of the 520 x 96 x 72 grid, a lossy bar through the layers: shell2 pairs / single steps / shell2 pairs with
    other shapes — an odd number of pairs per run"""
    bspec = td.BoundarySpec(x=td.Boundary(minus=td.PML(num_layers=5), plus=td.PML(num_layers=3)), y=td.Boundary.pml(num_layers=4),
                            z=td.Boundary(minus=td.PML(num_layers=3), plus=td.PML(num_layers=5)))
    bar = [td.Structure(geometry=td.Box(center=(-1.0, 0, 0), size=(td.inf, 0.8, 0.6)), medium=td.Medium(permittivity=3.0, conductivity=0.02))]
    sim = _sim(structures=bar, bspec=bspec)
    sim = sim.updated_copy(sources=[s for q, s in enumerate(sim.sources) if q != 2])      # (the dipole next to the x-max layers would keep the shell on single steps)
    spec = lc.spec_of(sim, 54)
    A = {L.OPT_SHELL_PAIRS: -1, L.OPT_SHELL2: 1, L.OPT_DEBUG_SYNC: 0}
    B = {L.OPT_SHELL_PAIRS: 0, L.OPT_SHELL2: 0, L.OPT_DEBUG_SYNC: 1}
    Cc = {L.OPT_SHELL_PAIRS: 2, L.OPT_SHELL2: 2, L.OPT_SHELL2_SHAPE: 32 + 128 * 4, L.OPT_STRIP: 8 + 64 * 4, L.OPT_DEBUG_SYNC: 0}
    rows, _ = lc.switched("device: SHELL_PAIRS/SHELL2/SHAPE/STRIP/DEBUG_SYNC", spec, hip_lib, DEV | {L.OPT_TWOSTEP: W16}, [A, B, Cc], 18, seed=7, z_chunk=0)
    assert [c["fused2_pairs"] for c in rows] == [9, 0, 9] and rows[1]["fused2_off_reason"] != 0, rows
    assert rows[0]["shell2_pairs"] == 9 and rows[1]["shell2_pairs"] == 0 and rows[2]["shell2_pairs"] == 9, rows


@pytest.mark.parametrize("workload", ["v2", "v3"])
def test_reset_equals_a_fresh_handle_on_the_bench_workloads(workload, hip_lib):
    """256^3, CPML (v2) and a Lorentz sphere in it (v3), random initial fields set again after the reset, the library's own choice of
    step pairs"""
    spec = _bench_spec(workload, 40)
    rows, *_ = lc.after_reset(f"device: reset ({workload} 256^3)", spec, hip_lib, DEV, 30, 40, seed=5, proof=lc.pairs_in_both(), z_chunk=0)
    if workload == "v3":
        assert rows[0]["disp_pairs"] > 0 and rows[1]["disp_pairs"] > 0, rows


def test_round_trip_with_paged_dispersive_cells(hip_lib):
    """lorentz_sphere at three times its size (the pairs advance its cells themselves): get_field / set_field of all six in mid-run"""
    fn = cases.lorentz_sphere
    spec = lc.spec_of(fn(tuple(3 * n for n in fn.__defaults__[0])), 60)
    got = lc.round_trip("device: round trip, paged dispersive cells", spec, hip_lib,
                        DEV | {L.OPT_TWOSTEP: 8 + 64 * 8, L.OPT_SHELL_PAIRS: 1, L.OPT_SHELL2: 1}, 25, 60, proof=lc.pairs_in_both("disp_pairs"), z_chunk=0)
    lc.held_to_oracle("device: get_field / set_field", spec, got)
