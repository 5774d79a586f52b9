"""Projection-monitor surfaces accumulated on their sampling lattice only, on the device: the case and the checks of
tests/test_emu_projection_dft.py on the product library (against the host path, against the fp64 oracle, the projected fields and
files of web.run, bit for bit across schedules and axis renamings, the lifecycle, the refusals), and the schedules once more on the
520 x 96 x 72 grid of tests/flux_time_case.py — CPML on every face, three x tiles — where the two-step sweep and the shell's boxes copy
the middle step out and lattice_dft_record_kernel reads that dump: a plane normal to z across seam column 256, a plane normal to x
(the lanes along y, several workgroups), and a plane reaching into the z-max CPML.  No oracle run on that grid (it takes minutes)."""
import numpy as np
import pytest

from tidy3d_amd import lib as L
from tidy3d_amd.engine import HipEngine

import projection_dft_case as case
import test_emu_projection_dft as emu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(hip_lib):
    dd, dh = case.discs()
    raw_a, _ = case.run_engine(dd.spec, hip_lib)
    raw_b, _ = case.run_engine(dh.spec, hip_lib)
    return dict(dd=dd, dh=dh, raw_a=raw_a, raw_b=raw_b)


def test_the_feature_is_there(ctx, hip_lib):
    emu.test_the_feature_is_there(ctx, hip_lib)


def test_device_values_match_the_host_path(ctx):
    emu.test_device_values_match_the_host_path(ctx)


def test_device_values_match_the_oracle(ctx):
    emu.test_device_values_match_the_oracle(ctx)


def test_end_result_and_files(hip_lib, tmp_path):
    emu.end_result(hip_lib, tmp_path)


def test_values_are_bit_identical_across_schedules_and_axes(ctx, hip_lib):
    emu.test_values_are_bit_identical_across_schedules(ctx, hip_lib)
    for shift in (1, 2):
        emu.test_renamed_axes(ctx, hip_lib, shift)


def test_lifecycle_and_zero_weights(ctx, hip_lib):
    emu.test_late_monitor_reset_and_reads_in_mid_run(ctx, hip_lib)
    emu.nan_under_zero_weight(ctx["dd"].spec, hip_lib)


def test_refusals(hip_lib):
    emu.test_refusals(hip_lib)


def test_three_x_tiles_with_cpml_shell(hip_lib):
    dd, dh = case.discs(case.big_simulation(), case.BIG_STEPS)
    dd.spec.decay_every = dh.spec.decay_every = 0
    assert dd.spec.shape[0] == 528 and [m.kind for m in dd.spec.monitors] == ["dft_lattice"] * 3
    mons = {m.name.split("::")[0]: m for m in dd.spec.monitors}
    assert mons["seam_z"].lo[0] < 255 and mons["seam_z"].hi[0] > 257 and mons["seam_z"].targets[0][2] == 1 and mons["seam_z"].targets[0][0] > 64
    assert mons["plane_x"].targets[0][0] == 1 and mons["plane_x"].targets[0][1] > 64      # (lanes along y: more than one piece of 64)
    assert mons["shell"].hi[2] > dd.spec.shape[2] - 5               # (five layers on z max)
    dev = {L.OPT_PLACEMENT_TRIES: 0}
    ref, st = case.run_engine(dd.spec, hip_lib, opts=dev, z_chunk=0)
    assert int(st.fused2_pairs) == 0 and all(np.abs(v).max() > 0 for v in ref.values())
    host, _ = case.run_engine(dh.spec, hip_lib, opts=dev, z_chunk=0)
    a, b = case.lattice_values(dd, ref, case.BIG_NAMES), case.lattice_values(dh, host, case.BIG_NAMES)
    worst, at = case.worst_host_ratio(a, b, case.box_scales(dh, host, case.BIG_NAMES))
    print(f"[projection_dft] 520 x 96 x 72, device against host path: worst |dA - dB| / A = {worst / case.EPS32:.3f} x 2^-24 at {at}")
    assert worst <= case.HOST_BAR, (worst / case.EPS32, at)
    with HipEngine(dd.spec, lib=hip_lib) as e:
        for n in case.BIG_NAMES:
            assert e.monitor_bytes(n, detail=True)["series"] == case.lattice_bytes(dd, n), n
    got, st = case.run_engine(dd.spec, hip_lib, twostep=16 + 64 * 32, opts=dev | {L.OPT_SHELL_PAIRS: -1, L.OPT_SHELL2: 1}, z_chunk=0)
    print(f"[projection_dft] 520 x 96 x 72: fused2_pairs={int(st.fused2_pairs)} shell_pairs={int(st.shell_pairs)} shell2_pairs={int(st.shell2_pairs)}")
    assert int(st.fused2_pairs) > 0 and int(st.shell2_pairs) > 0, int(st.fused2_off_reason)
    case.same_bits(got, ref)
