"""Checkpoint and resume on the device: scenarios (a) to (h) of tests/checkpoint_case.py through the real library — at the emulator's
shapes where a section exists there, at 520 x 96 x 72 (deferred seam pairs of sixteen-wave launches) and three times lorentz_sphere
(paged dispersive cells) where it takes the device — web.run suspended and resumed, and a first slice taken in another process.
Every comparison is equality of bits."""
import dataclasses
import os

import pytest

import checkpoint_case as cc
import test_emu_checkpoint as tec
import test_emu_lifecycle as lc
from tidy3d_amd import lib as L
from tidy3d_amd import web
from tidy3d_amd.exceptions import RunSuspended

pytestmark = pytest.mark.gpu


def _device(case):
    """the emulator's settings of a small scenario, without the placement probe"""
    return dataclasses.replace(case, opts=case.opts | {L.OPT_PLACEMENT_TRIES: 0})


def _all_variants(name, case, lib):
    for v in tec._variants(case):
        for k in case.ks:
            cc.check(name, dataclasses.replace(case, proof=case.proof if v == "fused" else None), lib, v, k)


@pytest.mark.parametrize("n,k", [(7, 3), (8, 4)])
def test_a_cpml_and_lorentz_block(n, k, hip_lib):
    _all_variants("device a", _device(cc.scenario_a(n, (k,))), hip_lib)


@pytest.mark.parametrize("k", [6, 5])
def test_a_cpml_cut_between_shell2_pairs(k, hip_lib):
    case = _device(cc.scenario_a_pairs(ks=(k,)))
    rows = cc.check("device a, shell2 pairs", case, hip_lib, "fused", k)
    assert rows[0]["shell2_pairs"] == k // 2, rows


def test_state_put_back_into_a_live_handle_that_has_paged(hip_lib):
    """fdtd_set_state rebuilds the paged memory terms with the set-up kernel: the bits ade_kernel / ade2_kernel left there (a Lorentz
    sphere and a two-pole Drude block, advanced inside shell2 pairs), and the psi sets of a handle in mid-ping-pong"""
    rows = cc.live_round_trip(cc.scenario_d("gpu"), hip_lib)
    assert rows[0]["disp_pairs"] > 0 and rows[1]["disp_pairs"] > 0, rows
    cc.live_round_trip(_device(cc.scenario_a_pairs()), hip_lib)


def test_b_deferred_seam_pairs_cut_on_an_odd_step(hip_lib):
    _all_variants("device b", cc.scenario_b("gpu"), hip_lib)


@pytest.mark.parametrize("oblique", [False, True])
def test_c_tfsf_lines_at_the_largest_injection(oblique, hip_lib):
    _all_variants(f"device c oblique={oblique}", _device(cc.scenario_c(oblique)), hip_lib)


def test_d_paged_memory_terms_into_a_handle_that_has_not_run(hip_lib):
    _all_variants("device d", cc.scenario_d("gpu"), hip_lib)


def test_e_one_monitor_of_every_kind(hip_lib):
    _all_variants("device e", _device(cc.scenario_e()), hip_lib)


def test_f_bloch_pair_with_a_fully_anisotropic_body(hip_lib):
    case = cc.scenario_f()
    cc.check("device f", case, hip_lib, "bloch", case.ks[0])


@pytest.mark.parametrize("kind", ["modulation", "conformal", "nonlinear"])
def test_g_whole_grid_lists_carry_no_state(kind, hip_lib):
    _all_variants(f"device g {kind}", _device(cc.scenario_g(kind)), hip_lib)


def test_h_shutoff_stops_at_the_same_step(hip_lib):
    case = _device(cc.scenario_h())
    ref = cc.uncut(case, hip_lib, "fused")
    stop = int(ref[2].steps_done)
    print(f"[checkpoint] device h: the uncut run stops at step {stop}, field_decay {ref[2].field_decay!r}")
    assert int(ref[2].stopped_early) == 1 and 12 <= stop < case.n and stop % case.spec.decay_every == 0
    for k in case.ks:
        got, st, rows, _ = cc.cut_and_resumed(case, hip_lib, "fused", k)
        lc.show(f"checkpoint device h cut at {k}", rows)
        cc.same_run(ref, got, st)
        assert int(st.steps_done) == stop and int(st.stopped_early) == 1


def test_web_run_suspends_and_resumes(hip_lib, tmp_path):
    sim = cc.web_scene()
    path = str(tmp_path / "run.state")
    ref = web.run(sim, verbose=False, n_steps=30)
    with pytest.raises(RunSuspended) as info:
        web.run(sim, verbose=False, n_steps=30, checkpoint=path, step_budget=11)
    assert info.value.step == 11 and os.path.exists(path)
    got = web.run(sim, verbose=False, n_steps=30, checkpoint=path)
    assert "Resumed from step 11 of 30" in got.log and not os.path.exists(path)
    cc.same_data(ref, got)
    every = web.run(sim, verbose=False, n_steps=30, checkpoint=path, checkpoint_steps=8)
    assert "Checkpoints written: 3" in every.log and not os.path.exists(path)
    cc.same_data(ref, every)


def test_resume_in_another_process(hip_lib, tmp_path):
    case = _device(cc.scenario_a())
    path = str(tmp_path / "child.state")
    tec.first_slice_in_a_child("", path)
    ref = cc.uncut(case, hip_lib, "fused")
    with cc.engine(case, hip_lib, "fused") as e:
        e.load_state(path, {"n_steps": case.n})
        assert int(e.stats().steps_done) == 3
        st = e.run(case.n - 3)
        cc.same_run(ref, cc.snapshot(e), st)
