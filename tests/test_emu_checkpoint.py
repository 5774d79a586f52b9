"""Checkpoint and resume on the emulated library: the C ABI (fdtd_state_fingerprint / fdtd_state_bytes / fdtd_get_state /
fdtd_set_state), HipEngine.save_state / load_state and web.run(checkpoint=...).  Scenarios and harness: tests/checkpoint_case.py;
every comparison is equality of bits (docs/history/CHECKPOINT.md has the table)."""
import ctypes as C
import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest

import tidy3d_amd.schema as td
from tidy3d_amd import lib as L
from tidy3d_amd import web
from tidy3d_amd.exceptions import RunSuspended, SetupError, SolverLibraryError, Tidy3dNotImplementedError

import checkpoint_case as cc
import test_emu_lifecycle as lc

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HEAD = C.sizeof(L.FdtdStateHeader)


# ------------------------------------------------------------------------------------------------------------------ the C ABI
def test_state_symbols_are_declared_and_bound(emu_lib):
    from test_capi_symbols import _declared
    names = {"fdtd_state_fingerprint", "fdtd_state_bytes", "fdtd_get_state", "fdtd_set_state"}
    assert names <= set(_declared()) & set(L.SYMBOLS)
    assert all(hasattr(emu_lib.dll, s) for s in names)
    assert HEAD == 96


def _header(blob):
    hd = L.FdtdStateHeader.from_buffer_copy(blob[:HEAD].tobytes())
    sec = np.frombuffer(blob[HEAD:HEAD + 8 * hd.n_sections].tobytes(), dtype=np.uint64)
    return hd, sec


def test_state_bytes_equal_the_sum_in_the_header(emu_lib):
    case = cc.scenario_a()
    with cc.engine(case, emu_lib, "fused", case.seed) as e:
        e.run(3)
        blob = e.get_state()
        hd, sec = _header(blob)
        n = int(e.lib.dll.fdtd_state_bytes(e.handle))
        assert hd.magic == L.STATE_MAGIC and hd.version == L.STATE_VERSION and hd.step == 3 and hd.fingerprint == e.state_fingerprint()
        assert n == blob.nbytes == hd.total_bytes == HEAD + 8 * hd.n_sections + 16 * hd.n_monitors + int(sec.sum())
        # six fields, E- and H-side psi of three axes (two arrays each), e_old and q of every ADE group, a time and a DFT monitor
        assert hd.n_sections > 20 and (hd.n_sections - 20) % 2 == 0 and hd.n_monitors == 2


def test_fingerprint_is_the_handles_and_not_the_steps(emu_lib):
    case = cc.scenario_a()
    with cc.engine(case, emu_lib, "fused", case.seed) as e:
        fp = e.state_fingerprint()
        e.run(3)
        assert e.state_fingerprint() == fp
        e.run(2)
        assert e.state_fingerprint() == fp
        e.reset()
        assert e.state_fingerprint() == fp
    with cc.engine(case, emu_lib, "twopass") as e:
        assert e.state_fingerprint() == fp           # (the variant is no part of the layout)


def _variants_of_a():
    base = cc._pml_lorentz_sim()
    pml5 = dataclasses.replace(base, boundary_spec=td.BoundarySpec(x=td.Boundary(minus=td.PML(num_layers=5), plus=td.PML(num_layers=4)),
                                                                   y=td.Boundary.pml(num_layers=4), z=td.Boundary.pml(num_layers=4)),
                               size=(base.size[0] - cc.DL, base.size[1], base.size[2]))
    more = dataclasses.replace(base, monitors=list(base.monitors) + [td.FieldTimeMonitor(center=(0, 0, 0), size=(0, 0, 0), name="p", colocate=False)])
    pole = dataclasses.replace(base, structures=[dataclasses.replace(base.structures[0], medium=td.Lorentz(eps_inf=2.0, coeffs=[(2.0, 4e14, 2e13), (1.0, 5e14, 3e13)]))])
    cell = dataclasses.replace(base, size=(base.size[0], base.size[1], base.size[2] + cc.DL))
    return {"one CPML layer": pml5, "one monitor": more, "one pole": pole, "one cell": cell}


def test_fingerprint_differs_with_the_layout(emu_lib):
    case = cc.scenario_a()
    with cc.engine(case, emu_lib, "fused") as e:
        fp = e.state_fingerprint()
    seen = {fp}
    for what, sim in _variants_of_a().items():
        spec = lc.spec_of(sim, 7)
        if what == "one CPML layer":
            assert spec.shape == case.spec.shape      # (the same padded grid: only the layer count differs)
        with cc.engine(dataclasses.replace(case, spec=spec), emu_lib, "fused") as e:
            other = e.state_fingerprint()
        assert other not in seen, what
        seen.add(other)


def _foreign_blob(emu_lib):
    spec = lc.spec_of(_variants_of_a()["one monitor"], 7)
    with cc.engine(dataclasses.replace(cc.scenario_a(), spec=spec), emu_lib, "fused", 3) as e:
        e.run(2)
        return e.get_state()


def test_every_refusal_leaves_the_handle_untouched(emu_lib):
    """bad magic, bad version, foreign fingerprint, a section of another size, a short buffer: named, and the run that follows equals the
    run of a handle that never saw the call"""
    case = cc.scenario_a()
    ref = cc.uncut(case, emu_lib, "fused")
    with cc.engine(case, emu_lib, "fused", case.seed) as e:
        e.run(3)
        good = e.get_state()
        hd, _ = _header(good)

        def edited(**kw):
            h2 = L.FdtdStateHeader.from_buffer_copy(good[:HEAD].tobytes())
            for k, v in kw.items():
                setattr(h2, k, v)
            out = good.copy()
            out[:HEAD] = np.frombuffer(bytes(h2), dtype=np.uint8)
            return out

        resized = good.copy()
        resized[HEAD:HEAD + 8] = np.frombuffer(np.uint64(int(_header(good)[1][0]) + 4).tobytes(), dtype=np.uint8)
        bad = {"bad magic": edited(magic=b"FDTDSTA9"), "format version": edited(version=L.STATE_VERSION + 1),
               "fingerprint": _foreign_blob(emu_lib), "fingerprint ": edited(fingerprint=hd.fingerprint ^ 1),
               "section 0 holds": resized, "too small": good[:good.nbytes - 4].copy(), "too small ": good[:40].copy()}
        e.run(1)
        for why, blob in bad.items():
            with pytest.raises(SolverLibraryError, match=why.strip()):
                e.set_state(blob)
            assert int(e.stats().steps_done) == 4
        st = e.run(case.n - 4)
        cc.same_run(ref, cc.snapshot(e), st)


def test_z_slab_handles_refuse_by_name(emu_lib):
    from tidy3d_amd.engine import HipEngine
    spec = lc.spec_of(cases_periodic(), 6)
    with HipEngine(spec, lib=emu_lib, force_comm=True) as e:
        e.comm_init(e.unique_id())
        for call in (e.state_fingerprint, e.get_state, lambda: e.set_state(np.zeros(200, np.uint8))):
            with pytest.raises(SolverLibraryError, match="state save / restore is not available on z-slab handles"):
                call()
        assert int(e.lib.dll.fdtd_state_bytes(e.handle)) < 0


def cases_periodic():
    import cases
    return cases.periodic_box_tall()


def test_state_put_back_into_the_live_handle_changes_no_bit(emu_lib):
    """get_state -> set_state on the same handle, in mid-run, on the scenario whose handle has paged its memory terms (fdtd_set_state
    rebuilds them from the pole states) and on the CPML / ADE box"""
    for case in (cc.scenario_d_live("emu"), cc.scenario_a(), cc.scenario_a_pairs()):
        cc.live_round_trip(case, emu_lib)


# ------------------------------------------------------------------------------------------------------------------ scenarios
def _variants(case):
    return ["fused"] + (["twopass"] if case.two_pass else [])


@pytest.mark.parametrize("n,k", [(7, 3), (8, 4)])
def test_a_cpml_and_lorentz_block(n, k, emu_lib):
    case = cc.scenario_a(n, (k,))
    for v in _variants(case):
        cc.check("a", case, emu_lib, v, k)          # (a CPML shell this large a part of the grid keeps single steps: the rows name the reason)


@pytest.mark.parametrize("k", [6, 5])
def test_a_cpml_cut_between_shell2_pairs(k, emu_lib):
    """the psi ping-pong of both sides: a cut behind an odd number of shell2 pairs, and behind pairs and a single step"""
    case = cc.scenario_a_pairs(ks=(k,))
    rows = cc.check("a, shell2 pairs", case, emu_lib, "fused", k)
    assert rows[0]["shell2_pairs"] == k // 2, rows


def test_b_deferred_seam_pairs_cut_on_an_odd_step(emu_lib):
    case = cc.scenario_b("emu")
    for v in _variants(case):
        cc.check("b", dataclasses.replace(case, proof=case.proof if v == "fused" else None), emu_lib, v, case.ks[0])


@pytest.mark.parametrize("oblique", [False, True])
def test_c_tfsf_lines_at_the_largest_injection(oblique, emu_lib):
    case = cc.scenario_c(oblique)
    for v in _variants(case):
        cc.check(f"c oblique={oblique}", case, emu_lib, v, case.ks[0])


def test_d_paged_memory_terms_into_a_handle_that_has_not_run(emu_lib):
    case = cc.scenario_d("emu")
    cc.check("d", case, emu_lib, "fused", case.ks[0])


def test_e_one_monitor_of_every_kind(emu_lib):
    case = cc.scenario_e()
    for v in _variants(case):
        cc.check("e", case, emu_lib, v, case.ks[0])


def test_f_bloch_pair_with_a_fully_anisotropic_body(emu_lib):
    case = cc.scenario_f()
    cc.check("f", case, emu_lib, "bloch", case.ks[0])


@pytest.mark.parametrize("kind", ["modulation", "conformal", "nonlinear"])
def test_g_whole_grid_lists_carry_no_state(kind, emu_lib):
    case = cc.scenario_g(kind)
    for v in _variants(case):
        cc.check(f"g {kind}", case, emu_lib, v, case.ks[0])


def test_h_shutoff_stops_at_the_same_step(emu_lib):
    case = cc.scenario_h()
    ref = cc.uncut(case, emu_lib, "fused")
    stop = int(ref[2].steps_done)
    print(f"[checkpoint] h: the uncut run stops at step {stop}, field_decay {ref[2].field_decay!r}")
    assert int(ref[2].stopped_early) == 1 and 12 <= stop < case.n and stop % case.spec.decay_every == 0
    for k in case.ks:
        got, st, rows, _ = cc.cut_and_resumed(case, emu_lib, "fused", k)
        lc.show(f"checkpoint h cut at {k}", rows)
        cc.same_run(ref, got, st)
        assert int(st.steps_done) == stop and int(st.stopped_early) == 1


# ------------------------------------------------------------------------------------------------------------ files of the engine
def test_state_file_round_trip_truncation_and_foreign_meta(emu_lib, tmp_path):
    case = cc.scenario_a()
    path = str(tmp_path / "a.state")
    meta = {"n_steps": case.n, "simulation": "abc"}
    ref = cc.uncut(case, emu_lib, "fused")
    got, st, rows, _ = cc.cut_and_resumed(case, emu_lib, "fused", 3, path=path, meta=meta)
    cc.same_run(ref, got, st)
    assert not os.path.exists(path + ".tmp")
    with cc.engine(case, emu_lib, "fused") as e:
        with pytest.raises(SetupError, match="meta 'simulation' differs"):
            e.load_state(path, dict(meta, simulation="abd"))
        with pytest.raises(SetupError, match="meta 'n_steps' differs"):
            e.load_state(path, dict(meta, n_steps=case.n + 1))
        raw = open(path, "rb").read()
        short = str(tmp_path / "short.state")
        open(short, "wb").write(raw[:-100])
        with pytest.raises(SetupError, match="truncated"):
            e.load_state(short, meta)
        open(short, "wb").write(raw[:20])
        with pytest.raises(SetupError, match="not a state file"):
            e.load_state(short, meta)
        assert int(e.stats().steps_done) == 0
    spec = lc.spec_of(_variants_of_a()["one monitor"], 7)
    with cc.engine(dataclasses.replace(case, spec=spec), emu_lib, "fused") as e:
        with pytest.raises(SetupError, match="fingerprint"):
            e.load_state(path, meta)


# ------------------------------------------------------------------------------------------------------------------- web.run
def _plain(sim, lib, **kw):
    return web.run(sim, verbose=False, lib=lib, **kw)


def test_web_run_suspends_and_resumes(emu_lib, tmp_path):
    sim = cc.web_scene()
    path = str(tmp_path / "run.state")
    ref = _plain(sim, emu_lib, n_steps=30)
    with pytest.raises(RunSuspended) as info:
        _plain(sim, emu_lib, n_steps=30, checkpoint=path, step_budget=11)
    assert info.value.step == 11 and info.value.path == path and os.path.exists(path)
    got = _plain(sim, emu_lib, n_steps=30, checkpoint=path, step_budget=30)
    assert "Resumed from step 11 of 30 (checkpoint '%s')" % path in got.log
    assert not os.path.exists(path)
    cc.same_data(ref, got)
    assert {"field", "flux_t", "mode"} <= set(got.monitor_data)


def test_web_run_three_slices_one_slice_and_periodic_writes(emu_lib, tmp_path):
    sim = cc.web_scene()
    ref = _plain(sim, emu_lib, n_steps=30)
    path = str(tmp_path / "three.state")
    steps = []
    for _ in range(2):
        with pytest.raises(RunSuspended) as info:
            _plain(sim, emu_lib, n_steps=30, checkpoint=path, step_budget=9)
        steps.append(info.value.step)
    assert steps == [9, 18]
    three = _plain(sim, emu_lib, n_steps=30, checkpoint=path, step_budget=12)
    one = _plain(sim, emu_lib, n_steps=30, checkpoint=str(tmp_path / "one.state"), step_budget=30)
    every = _plain(sim, emu_lib, n_steps=30, checkpoint=str(tmp_path / "every.state"), checkpoint_steps=8)
    assert "Checkpoints written: 3" in every.log and not os.listdir(str(tmp_path))
    for got in (three, one, every):
        cc.same_data(ref, got)


def test_web_run_shutoff_is_met_at_the_same_step(emu_lib, tmp_path):
    """a lossy scene that stops early: the chunks end on other steps than the decay checks, the run stops where the plain call stops"""
    base = cc.web_scene(run_time=2e-13)
    lossy = td.Structure(geometry=td.Box(center=(0, 0, 0), size=(td.inf, td.inf, td.inf)), medium=td.Medium(permittivity=1.0, conductivity=0.5))
    sim = dataclasses.replace(base, structures=[lossy] + list(base.structures), shutoff=1e-2)
    ref = _plain(sim, emu_lib)
    line = [ln for ln in ref.log.splitlines() if "exiting solver" in ln]
    assert line, ref.log
    got = _plain(sim, emu_lib, checkpoint=str(tmp_path / "s.state"), checkpoint_steps=7)
    assert [ln for ln in got.log.splitlines() if "exiting solver" in ln] == line and got.final_decay_value == ref.final_decay_value
    assert [ln for ln in got.log.splitlines() if ln.startswith("- Time step")] == [ln for ln in ref.log.splitlines() if ln.startswith("- Time step")]
    cc.same_data(ref, got)


def test_web_run_refuses_a_file_of_another_simulation_and_bad_keywords(emu_lib, tmp_path):
    sim = cc.web_scene()
    path = str(tmp_path / "old.state")
    with pytest.raises(RunSuspended):
        _plain(sim, emu_lib, n_steps=20, checkpoint=path, step_budget=5)
    before = open(path, "rb").read()
    other = dataclasses.replace(sim, structures=[dataclasses.replace(sim.structures[0], medium=td.Medium(permittivity=4.5))])
    with pytest.raises(SetupError, match="meta 'simulation' differs"):
        _plain(other, emu_lib, n_steps=20, checkpoint=path)
    with pytest.raises(SetupError, match="meta 'n_steps' differs"):
        _plain(sim, emu_lib, n_steps=21, checkpoint=path)
    assert open(path, "rb").read() == before
    with pytest.raises(Tidy3dNotImplementedError, match="without checkpoint="):
        _plain(sim, emu_lib, n_steps=20, step_budget=5)
    with pytest.raises(Tidy3dNotImplementedError, match="without checkpoint="):
        _plain(sim, emu_lib, n_steps=20, checkpoint_steps=5)
    with pytest.raises(Tidy3dNotImplementedError, match="without checkpoint="):
        _plain(sim, emu_lib, n_steps=20, time_budget=5.0)
    with pytest.raises(Tidy3dNotImplementedError, match="checkpoint_steps=0"):
        _plain(sim, emu_lib, n_steps=20, checkpoint=path, checkpoint_steps=0)
    with pytest.raises(Tidy3dNotImplementedError, match="more than one GPU"):
        _plain(sim, emu_lib, n_steps=20, checkpoint=path, devices=[0, 1])


def _custom_scene(scale):
    """web_scene with a CustomMedium block whose permittivity dataset is `scale` times a fixed 3 x 3 x 3 array (same coordinates, same
    shape and dtype: the handle's fingerprint cannot tell two scales apart)"""
    from tidy3d_amd.data import DataArray
    x = np.array([-0.1, 0.0, 0.1])
    eps = scale * (2.0 + 0.1 * np.arange(27, dtype=np.float64).reshape(3, 3, 3))
    arr = DataArray(eps, {"x": x, "y": x, "z": x})
    arr.tag = "SpatialDataArray"
    block = td.Structure(geometry=td.Box(center=(0, 0, 0), size=(0.2, 0.2, 0.2)), medium=td.CustomMedium(permittivity=arr, interp_method="nearest"))
    sim = cc.web_scene()
    return dataclasses.replace(sim, structures=list(sim.structures) + [block])


def test_web_run_refuses_an_old_file_when_only_a_dataset_changed(emu_lib, tmp_path):
    """the values of a CustomMedium dataset are part of the file's simulation hash (byte for byte; so are its coordinates)"""
    from tidy3d_amd.data import DataArray
    path = str(tmp_path / "custom.state")
    sim = _custom_scene(1.0)
    with pytest.raises(RunSuspended):
        _plain(sim, emu_lib, n_steps=12, checkpoint=path, step_budget=5)
    before = open(path, "rb").read()
    with pytest.raises(SetupError, match="meta 'simulation' differs"):
        _plain(_custom_scene(1.5), emu_lib, n_steps=12, checkpoint=path)
    assert open(path, "rb").read() == before
    ref = _plain(sim, emu_lib, n_steps=12)
    got = _plain(_custom_scene(1.0), emu_lib, n_steps=12, checkpoint=path)      # (an equal dataset in another object resumes)
    assert "Resumed from step 5 of 12" in got.log
    cc.same_data(ref, got)
    # the hash itself: values, coordinates, dtype; and nothing is ever hashed by its repr
    import hashlib

    def digest(v):
        h = hashlib.sha256()
        web._hash_value(h, v)
        return h.hexdigest()

    x = np.array([0.0, 1.0])
    base = DataArray(np.ones((2, 2, 2)), {"x": x, "y": x, "z": x})
    seen = {digest({"a": base})}
    for other in (DataArray(np.ones((2, 2, 2)) * (1 + 2e-16), {"x": x, "y": x, "z": x}), DataArray(np.ones((2, 2, 2)), {"x": x + 1e-9, "y": x, "z": x}),
                  DataArray(np.ones((2, 2, 2), np.float32), {"x": x, "y": x, "z": x}), np.ones((2, 2, 2))):
        d = digest({"a": other})
        assert d not in seen
        seen.add(d)
    assert digest({"a": DataArray(np.ones((2, 2, 2)), {"x": x.copy(), "y": x, "z": x})}) == digest({"a": base})
    with pytest.raises(Tidy3dNotImplementedError, match="cannot tie a state file"):
        digest({"a": object()})


def test_web_run_does_not_write_the_same_step_twice(emu_lib, tmp_path, monkeypatch):
    """a step budget that ends on a multiple of checkpoint_steps: the periodic write is the suspend's file"""
    from tidy3d_amd.engine import HipEngine
    steps, real = [], HipEngine.save_state

    def counted(self, path, meta, extra=None):
        steps.append(real(self, path, meta, extra=extra))
        return steps[-1]

    monkeypatch.setattr(HipEngine, "save_state", counted)
    path = str(tmp_path / "twice.state")
    with pytest.raises(RunSuspended) as info:
        _plain(cc.web_scene(), emu_lib, n_steps=20, checkpoint=path, checkpoint_steps=5, step_budget=10)
    assert info.value.step == 10 and steps == [5, 10]
    with pytest.raises(RunSuspended):
        _plain(cc.web_scene(), emu_lib, n_steps=20, checkpoint=path, step_budget=0)      # (nothing taken: the file already holds step 10)
    assert steps == [5, 10]
    got = _plain(cc.web_scene(), emu_lib, n_steps=20, checkpoint=path)
    cc.same_data(_plain(cc.web_scene(), emu_lib, n_steps=20), got)


def test_load_state_never_leaves_a_bloch_pair_half_restored(emu_lib, tmp_path, monkeypatch):
    """should the library fail on the twin's blob, both handles are back at step 0"""
    from tidy3d_amd.engine import HipEngine
    case = cc.scenario_f()
    path = str(tmp_path / "pair.state")
    with cc.engine(case, emu_lib, "bloch") as e:
        e.run(5)
        e.save_state(path, {})
    with cc.engine(case, emu_lib, "bloch") as e:
        real = HipEngine.set_state

        def failing(self, blob):
            if self is e.twin:
                raise SolverLibraryError("fdtd_set_state failed: injected")
            return real(self, blob)

        monkeypatch.setattr(HipEngine, "set_state", failing)
        with pytest.raises(SetupError, match="both handles of the pair were reset"):
            e.load_state(path, {})
        assert int(e.stats().steps_done) == 0 and int(e.twin.stats().steps_done) == 0
        monkeypatch.setattr(HipEngine, "set_state", real)
        ref = cc.uncut(case, emu_lib, "bloch")
        st = e.run(case.n)
        cc.same_run(ref, cc.snapshot(e), st)


# ------------------------------------------------------------------------------------------------------------ across processes
CHILD = """
import sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
from tidy3d_amd.lib import load_library
import checkpoint_case as cc
case = cc.scenario_a()
lib = load_library({lib!r}) if {lib!r} else load_library()
with cc.engine(case, lib, "fused", case.seed) as e:
    e.run(3)
    assert e.save_state({path!r}, {{"n_steps": case.n}}) == 3
print("saved")
"""


def first_slice_in_a_child(lib_path, path):
    """scenario (a): 3 steps and save_state in a fresh child process (one at a time, no exec)"""
    code = CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), lib=lib_path, path=path)
    out = subprocess.run([sys.executable, "-c", code], timeout=240, capture_output=True, text=True)
    assert out.returncode == 0 and "saved" in out.stdout, (out.returncode, out.stdout[-2000:], out.stderr[-2000:])


def test_resume_in_another_process(emu_lib, tmp_path):
    case = cc.scenario_a()
    path = str(tmp_path / "child.state")
    first_slice_in_a_child(emu_lib.path, path)
    ref = cc.uncut(case, emu_lib, "fused")
    with cc.engine(case, emu_lib, "fused") as e:
        e.load_state(path, {"n_steps": case.n})
        assert int(e.stats().steps_done) == 3
        st = e.run(case.n - 3)
        cc.same_run(ref, cc.snapshot(e), st)
