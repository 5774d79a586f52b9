"""FluxTimeMonitor surfaces reduced on the device, on the device: the case and the checks of tests/test_emu_flux_time.py on the
product library (against the host path, against the fp64 oracle, bit for bit across schedules and staging rings), and the schedules
once more on the 520 x 96 x 72 grid of tests/test_gpu_lifecycle.py — CPML on every face, three x tiles — where the two-step sweep,
the shell's boxes and the reduction all run, the records coming from launches on two streams: a small x-normal plane through the seam
column 256 that the sweep samples itself, a large one through the same column, a plane next to the z-max layers inside the shell,
and the x-z cross-section through all layers.  A missing edge between a record's writer and the reduction shows as differing bits."""
import numpy as np
import pytest

from tidy3d_amd import lib as L
from tidy3d_amd.discretize import discretize

import flux_time_case as case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(hip_lib):
    dd, dh = case.discs()
    raw_a, _ = case.run_engine(dd.spec, hip_lib)
    raw_b, _ = case.run_engine(dh.spec, hip_lib)
    return dict(dd=dd, dh=dh, raw_a=raw_a, raw_b=raw_b, scale=case.scales(dh, raw_b))


def test_device_series_match_the_host_path(ctx):
    a, b = case.series(ctx["dd"], ctx["raw_a"]), case.series(ctx["dh"], ctx["raw_b"])
    worst, at = case.worst_ratio(a, b, ctx["scale"])
    print(f"[flux_time] device against host path: worst |dA - dB| / A_scale = {worst / case.EPS32:.3f} x 2^-24 at '{at}' (bar 32 x 2^-24)")
    assert all(np.abs(b[n]).max() > 0 for n in case.NAMES)
    assert worst <= case.HOST_BAR, (worst / case.EPS32, at)


def test_device_series_match_the_oracle(ctx):
    from oracle.fdtd_numpy import OracleFdtd
    ref = case.series(ctx["dh"], OracleFdtd(ctx["dh"].spec).run())
    worst, at = case.worst_ratio(case.series(ctx["dd"], ctx["raw_a"]), ref, ctx["scale"])
    print(f"[flux_time] device against the fp64 oracle: worst |dA - oracle| / A_scale = {worst:.3e} at '{at}' (bar {case.ORACLE_BAR:.0e})")
    assert worst <= case.ORACLE_BAR, (worst, at)


def test_series_are_bit_identical_across_schedules_and_rings(ctx, hip_lib):
    two_pass, st = case.run_engine(ctx["dd"].spec, hip_lib, variant=L.VARIANT_ZMARCH)
    assert int(st.fused2_pairs) == 0
    case.same_bits(two_pass, ctx["raw_a"])
    pairs, st = case.run_engine(ctx["dd"].spec, hip_lib, twostep=case.TWOSTEP_WORD)
    assert int(st.fused2_pairs) > 0, int(st.fused2_off_reason)
    case.same_bits(pairs, ctx["raw_a"])
    for records in (2, 5):
        spec = case.with_budget(ctx["dd"].spec, records)
        case.same_bits(case.run_engine(spec, hip_lib)[0], ctx["raw_a"])
        got, st = case.run_engine(spec, hip_lib, twostep=case.TWOSTEP_WORD)
        assert int(st.fused2_pairs) > 0
        case.same_bits(got, ctx["raw_a"])


def test_three_x_tiles_with_cpml_shell(hip_lib):
    n_steps = case.BIG_STEPS
    dd = discretize(case.big_simulation(), n_steps=n_steps, flux_time_device=True)
    dd.spec.decay_every = 0
    assert dd.spec.shape[0] == 528
    small = [m for m in dd.spec.monitors if m.name.startswith("seam_small")][0]
    assert small.lo[0] <= 255 and small.hi[0] > 256 and 4 * int(np.prod(small.shape)) <= 1024, (small.lo, small.hi)
    dev = {L.OPT_PLACEMENT_TRIES: 0}
    ref, st = case.run_engine(dd.spec, hip_lib, opts=dev, z_chunk=0)
    assert int(st.fused2_pairs) == 0 and all(np.abs(v).max() > 0 for v in ref.values())
    spec5 = case.with_budget(dd.spec, 5)
    for spec in (dd.spec, spec5):
        got, st = case.run_engine(spec, hip_lib, twostep=16 + 64 * 32, opts=dev | {L.OPT_SHELL_PAIRS: -1, L.OPT_SHELL2: 1}, z_chunk=0)
        print(f"[flux_time] 520 x 96 x 72: fused2_pairs={int(st.fused2_pairs)} shell_pairs={int(st.shell_pairs)} shell2_pairs={int(st.shell2_pairs)}")
        assert int(st.fused2_pairs) > 0 and int(st.shell_pairs) > 0, int(st.fused2_off_reason)
        case.same_bits(got, ref)
    two_pass, _ = case.run_engine(dd.spec, hip_lib, variant=L.VARIANT_ZMARCH, opts=dev)
    case.same_bits(two_pass, ref)


def test_renamed_axes_and_web_run(ctx, hip_lib):
    """the engine's cyclic axis renaming (what best_axis_shift chooses on real grids) and the public entry point"""
    from tidy3d_amd import web
    for shift in (1, 2):
        raw, _ = case.run_engine(ctx["dd"].spec, hip_lib, axis_shift=shift)
        worst, at = case.worst_ratio(case.series(ctx["dd"], raw), case.series(ctx["dh"], ctx["raw_b"]), ctx["scale"])
        assert worst <= case.HOST_BAR, (shift, worst / case.EPS32, at)
    sd = web.run(case.simulation(), n_steps=case.N_STEPS, lib=hip_lib, verbose=False, flux_time_device=True, return_tidy3d=False)
    assert "FluxTimeMonitor reduced on the device: box, px, py, pz, win." in sd.log
    got = {n: np.asarray(sd[n].flux.values) for n in case.NAMES}
    worst, at = case.worst_ratio(got, case.series(ctx["dh"], ctx["raw_b"]), ctx["scale"])
    assert worst <= case.HOST_BAR, (worst / case.EPS32, at)
