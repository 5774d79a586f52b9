"""``run()``: local, MI355X-native drop-in for ``tidy3d.web.run``.

Mirrors the signature and behaviour of reference web/api/webapi.py:49-155 (via
web/api/autograd/autograd.py:86): takes the Simulation positionally, tolerates and ignores the
cloud-only keyword arguments, validates (``validate_pre_upload``, simulation.py:3341), runs the
solve — here on the local GPU through ``libfdtd_hip.so`` instead of upload/start/monitor/
download — and returns a ``SimulationData``; the post-run warnings of
``Tidy3dStubData.postprocess`` (web/api/tidy3d_stub.py:219-233) are replicated.  The test-suite
seam of the reference is ``monkeypatch.setattr(td.web, "run", run_emulated)``
(tests/utils.py:880, tests/test_plugins/test_adjoint.py:95); this function plugs into the same
seam.
"""
from __future__ import annotations

import json
import logging
import os
import time
from typing import Optional

import numpy as np

from . import schema as td
from .data import SimulationData, assemble
from .discretize import DevicePaths, _device_refusals, discretize
from .exceptions import SetupError, SolverLibraryError, Tidy3dNotImplementedError

log = logging.getLogger("tidy3d_amd")


def _as_mirror(simulation):
    """Accept a mirror Simulation, a real tidy3d.Simulation (anything with .json()/.dict()), a
    dict in tidy3d's JSON form, or a path to a .json file."""
    if isinstance(simulation, td.Simulation):
        return simulation, False
    if isinstance(simulation, str):
        return td.Simulation.from_file(simulation), False
    if isinstance(simulation, dict):
        return td.Simulation.from_dict(simulation), False
    if hasattr(simulation, "json") and callable(simulation.json):
        text = simulation.json()
        if 'DataArray"' in text and hasattr(simulation, "to_file"):
            # dataset-defined objects (custom media / sources, triangle meshes): the JSON form holds only
            # placeholders, the data go through the reference's own .hdf5 writer (ref base.py:364-420)
            import os
            import tempfile
            with tempfile.TemporaryDirectory() as tmp:
                fname = os.path.join(tmp, "simulation.hdf5")
                simulation.to_file(fname)
                return td.Simulation.from_file(fname), True
        return td.Simulation.from_dict(json.loads(text)), True
    raise SetupError(f"cannot interpret {type(simulation)!r} as a tidy3d Simulation")


def schedule_line(stats, n_cells: float, solve_s: float) -> str:
    """Which path the run took: the schedule, the step pairs taken of the steps run, why the rest (or all)
    went out as single steps, and the rate — a user cannot otherwise tell which of 190 / 140 / 125 / 95 Gcells/s a simulation gets."""
    from .lib import F2_OFF_REASONS
    steps = int(stats.steps_done)
    pairs, shell, shell2 = int(stats.fused2_pairs), int(stats.shell_pairs), int(stats.shell2_pairs)
    disp = int(getattr(stats, "disp_pairs", 0))
    rate = n_cells * steps / max(solve_s, 1e-9) / 1e9
    if not pairs:
        why = int(stats.fused2_off_reason)
        reason = F2_OFF_REASONS.get(why, f"reason {why}") if why else "fewer than two steps"
        return f"Schedule: one time step per sweep ({reason}); {rate:.1f} Gcells/s."
    if shell2:
        form = "two-step sweep over the bulk, the CPML shell two steps per sweep beside it"
    elif shell:
        form = "two-step sweep over the bulk, the CPML / periodic shell by single steps beside it"
    else:
        form = "two-step sweep over the whole grid"
    parts = [f"Schedule: two time steps per sweep ({form}) for {2 * pairs} of {steps} steps"]
    if disp:
        parts.append(f"dispersive cells advanced inside {disp} of the {pairs} pairs")
    single = steps - 2 * pairs
    if single > 0:
        why = int(getattr(stats, "single_step_reason", 0))
        parts.append(f"{single} single steps" + (f" ({F2_OFF_REASONS.get(why, f'reason {why}')})" if why and single > 2 else ""))
    return "; ".join(parts) + f"; {rate:.1f} Gcells/s."


def _log_line(step: int, n_steps: int, t: float, decay: float) -> str:
    """Format pinned by ref tests/test_data/test_sim_data.py:69,201-204."""
    perc = int(100 * step / max(n_steps, 1))
    mant = f"{decay:.3e}"
    return f"- Time step {step:6d} / time {t:.2e}s ({perc:3d} % done), field decay: {mant}"


CHECKPOINT_TIME_CHUNK = 1000       # time_budget without checkpoint_steps: the clock is read every that many time steps


def _hash_value(h, v, where="simulation") -> None:
    """Feed ``v`` — anything the mirror simulation's ``dict()`` can hold — into the hash ``h`` in a canonical form: mappings by sorted
    key, sequences in order, numbers by their exact value, arrays and datasets (anything with ``values`` and ``coords``: custom media,
    custom sources, modulation amplitudes) by dtype, shape and BYTES of the values and of every coordinate.  Nothing is ever hashed
    by its ``repr``: an object this walk does not know is refused (``Tidy3dNotImplementedError``), since a state file must not be
    accepted for a simulation that differs in something the hash did not see."""
    import dataclasses

    def tag(t, payload=b""):
        h.update(t.encode("ascii") + b":" + str(len(payload)).encode("ascii") + b":")
        h.update(payload)

    if v is None or isinstance(v, (bool, np.bool_)):
        tag("c", repr(None if v is None else bool(v)).encode("ascii"))
    elif isinstance(v, (int, np.integer)):
        tag("i", str(int(v)).encode("ascii"))
    elif isinstance(v, (float, np.floating)):
        tag("f", float(v).hex().encode("ascii"))
    elif isinstance(v, (complex, np.complexfloating)):
        tag("z", (float(v.real).hex() + "," + float(v.imag).hex()).encode("ascii"))
    elif isinstance(v, str):
        tag("s", v.encode("utf-8"))
    elif isinstance(v, bytes):
        tag("b", v)
    elif isinstance(v, dict):
        tag("d", str(len(v)).encode("ascii"))
        for k in sorted(v, key=str):
            tag("k", str(k).encode("utf-8"))
            _hash_value(h, v[k], f"{where}.{k}")
    elif isinstance(v, (list, tuple)):
        tag("l", str(len(v)).encode("ascii"))
        for q, x in enumerate(v):
            _hash_value(h, x, f"{where}[{q}]")
    elif isinstance(v, np.ndarray):
        if v.dtype.kind not in "biufc":
            raise Tidy3dNotImplementedError(f"checkpoint=: cannot tie a state file to {where}, an array of dtype {v.dtype}")
        a = np.ascontiguousarray(v)
        tag("a", (a.dtype.str + str(a.shape)).encode("ascii"))
        tag("v", a.tobytes())
    elif hasattr(v, "values") and hasattr(v, "coords") and not callable(getattr(v, "values")):       # a dataset array, ours or xarray's
        tag("D", str(getattr(v, "tag", type(v).__name__)).encode("utf-8"))
        _hash_value(h, [str(d) for d in getattr(v, "dims", ())], where + ".dims")
        coords = v.coords
        for d in sorted(coords, key=str):
            tag("k", str(d).encode("utf-8"))
            _hash_value(h, np.asarray(getattr(coords[d], "values", coords[d])), f"{where}.coords[{d}]")
        _hash_value(h, np.asarray(v.values), where + ".values")
    elif hasattr(v, "dict") and callable(v.dict):
        tag("m", type(v).__name__.encode("utf-8"))
        _hash_value(h, v.dict(), where)
    elif hasattr(v, "raw") and type(v).__name__ == "Unsupported":
        tag("u")
        _hash_value(h, v.raw, where)
    elif dataclasses.is_dataclass(v) and not isinstance(v, type):
        tag("o", type(v).__name__.encode("utf-8"))
        _hash_value(h, {f.name: getattr(v, f.name) for f in dataclasses.fields(v)}, where)
    else:
        raise Tidy3dNotImplementedError(f"checkpoint=: cannot tie a state file to {where}, an object of type "
                                        f"{type(v).__name__} (its contents would not be part of the file's simulation hash)")


def _checkpoint_meta(sim, spec, mode_grid_dispersion, lib) -> dict:
    """What a state file is tied to besides the handle's own fingerprint: the simulation (a hash of its ``dict()`` in the canonical
    form of ``_hash_value``: dataset values and coordinates byte for byte), the run length, the device-path choices as RESOLVED —
    the kind every monitor of ``spec`` came out as under the ``*_device`` keywords and thresholds (two calls whose keywords differ
    but resolve alike share a file) — the mode-source choice and the state-file ABI."""
    import hashlib
    from . import lib as L
    from .discretize import MODE_SOURCE_GRID_DISPERSION
    h = hashlib.sha256()
    _hash_value(h, sim.dict())
    return {"simulation": h.hexdigest(), "n_steps": int(spec.n_steps),
            "device_paths": [[m.name, m.kind] for m in spec.monitors],
            "mode_grid_dispersion": bool(MODE_SOURCE_GRID_DISPERSION if mode_grid_dispersion is None else mode_grid_dispersion),
            "abi": L.ABI_VERSION, "library": os.path.basename(lib.path)}


_PAIR_COUNTERS = ("fused2_pairs", "shell_pairs", "shell2_pairs", "disp_pairs", "src_paged_pairs")


def _run_in_chunks(eng, spec, progress, lines, verbose, path, meta, checkpoint_steps, step_budget, time_budget):
    """The solve of ``run(..., checkpoint=path)``: a sequence of ``eng.run(chunk)`` calls from the step a matching state file holds
    (or 0) to the last step, the state written at every multiple of ``checkpoint_steps`` and when a budget ends the call
    (``RunSuspended``).  The library checks the field decay on the handle's GLOBAL step count (``step % decay_every``,
    csrc/fdtd_run.hpp ``Run::decay_at``), so a chunk boundary may fall on any step: a chunked run meets the same checks at the same
    steps as a whole one, and ``checkpoint_steps`` is used as given.  -> (stats of the whole run, solve seconds of all calls)."""
    from .exceptions import RunSuspended
    n_steps = int(spec.n_steps)
    every = None if checkpoint_steps is None else int(checkpoint_steps)
    step, solve_before, sums = 0, 0.0, dict.fromkeys(_PAIR_COUNTERS, 0)
    in_file = None                                        # the step the file at `path` holds, where this call knows it

    def say(ln):
        lines.append(ln)
        if verbose:
            print(ln, flush=True)

    if os.path.exists(path):
        head = eng.load_state(path, meta)               # (SetupError names what differs; the file stays)
        extra = head.get("extra", {})
        step, solve_before = int(head["step"]), float(extra.get("solve_s", 0.0))
        in_file = step
        sums.update({k: int(v) for k, v in extra.get("pairs", {}).items() if k in sums})
        lines.extend(extra.get("log", []))
        say(f"Resumed from step {step} of {n_steps} (checkpoint '{path}')")
    if every is not None:
        say(f"Checkpoint every {every} time steps to '{path}' (field-decay checks count the run's own steps: no rounding needed)")
    n_head = len(lines)

    def save():
        keep = [ln for ln in lines[n_head:] if ln.startswith("- Time step")]
        t = time.perf_counter()
        eng.save_state(path, meta, extra={"solve_s": solve_before + (t - t0), "pairs": sums, "log": head_log + keep})
        return time.perf_counter() - t

    head_log = [ln for ln in lines[:n_head] if ln.startswith("- Time step")]
    t0 = time.perf_counter()
    taken, stats, save_s, n_saves = 0, eng.stats(), 0.0, 0
    while step < n_steps:
        chunk = n_steps - step
        if every is not None:
            chunk = min(chunk, every - step % every)
        elif time_budget is not None:
            chunk = min(chunk, CHECKPOINT_TIME_CHUNK)
        if step_budget is not None:
            chunk = min(chunk, int(step_budget) - taken)
        if chunk <= 0 or (time_budget is not None and time.perf_counter() - t0 >= float(time_budget)):
            if in_file != step:                           # (a budget that ends on a periodic write, or on the step resumed from: the file holds it)
                save()
            raise RunSuspended(path, step, n_steps)
        stats = eng.run(chunk, progress=progress)
        for k in _PAIR_COUNTERS:
            sums[k] += int(getattr(stats, k))
        taken += chunk
        step = int(stats.steps_done)
        if stats.stopped_early or stats.diverged:
            break
        if every is not None and step < n_steps and step % every == 0:
            save_s += save()
            n_saves += 1
            in_file = step
    for k in _PAIR_COUNTERS:                              # the schedule line speaks of the whole run
        setattr(stats, k, sums[k])
    if n_saves:
        say(f"Checkpoints written: {n_saves} ({save_s:.4f} s)")
    if os.path.exists(path):
        os.remove(path)
    return stats, solve_before + (time.perf_counter() - t0)


def run(simulation, task_name: Optional[str] = None, folder_name: str = "default",
        path: Optional[str] = None, callback_url: Optional[str] = None, verbose: bool = True,
        progress_callback_upload=None, progress_callback_download=None,
        solver_version: Optional[str] = None, worker_group: Optional[str] = None,
        simulation_type: str = "tidy3d", parent_tasks=None, local_gradient: bool = False,
        *, device: int = 0, n_steps: Optional[int] = None, lib=None,
        return_tidy3d: Optional[bool] = None, devices=None, _dist_options: Optional[dict] = None,
        mode_grid_dispersion: Optional[bool] = None, flux_time_device: Optional[bool] = None,
        field_time_device: Optional[bool] = None, field_dft_device: Optional[bool] = None,
        projection_device: Optional[bool] = None, exact_projection_device: Optional[bool] = None,
        rasterize_device: Optional[bool] = None, checkpoint: Optional[str] = None, checkpoint_steps: Optional[int] = None,
        step_budget: Optional[int] = None, time_budget: Optional[float] = None) -> SimulationData:
    """Solve ``simulation`` on the local MI355X and return its ``SimulationData``.

    Cloud-only arguments (``folder_name``, ``callback_url``, ``progress_callback_*``,
    ``solver_version``, ``worker_group``, ``parent_tasks``, ``local_gradient``) are accepted and
    ignored.  ``path``: when given, the data is written there — ``*.hdf5`` in the reference's file
    layout (loadable with ``tidy3d.SimulationData.from_file``), any other name as ``.npz``.  Extra keyword-only arguments select the GPU
    (``device``), override the number of time steps (``n_steps``, tests/benchmarks) or pass an
    explicitly loaded library (``lib``, tests).  ``devices=[0, 1, ...]``: one worker process per listed GPU, the
    grid split into z-slabs with RCCL ghost-plane exchange (``tidy3d_amd.dist``) — the whole multi-GPU run is this
    one call.  ``mode_grid_dispersion``: False launches mode sources with the continuum mode instead of the one the Yee
    grid propagates (``discretize.MODE_SOURCE_GRID_DISPERSION``, default True; one-GPU runs).  ``flux_time_device``: reduce
    ``FluxTimeMonitor`` surfaces on the device (True), on the host from plane records (False), or per monitor by the memory the
    records would take (None, ``discretize.FLUX_TIME_HOST_BYTES``; one-GPU runs without symmetry or Bloch boundaries).
    ``field_time_device``: colocate and downsample (``interval_space``) ``FieldTimeMonitor`` records on the device (True), on the host
    from records of the whole box (False), or per monitor (None: on the device where those records would exceed the same
    threshold and fewer nodes are kept than the box holds; the same kinds of run).  ``field_dft_device``: the same three values for
    ``FieldMonitor`` — accumulate its running DFT on the kept nodes only, on the device (True), over the whole box with colocation
    and ``interval_space`` on the host (False), or per monitor (None: on the device where the whole box's accumulators would
    exceed the threshold and fewer nodes are kept).  ``projection_device``: the same three values for the field projection monitors
    (angle, Cartesian, k-space, and ``DirectivityMonitor``, whose flux is then reduced on the device too) — accumulate every surface on its sampling lattice of 10 points per wavelength only, on the device
    (True), over the whole padded surface boxes with colocation and resampling on the host (False), or per monitor (None: on the
    device where the whole-box accumulators of all its surfaces would exceed the threshold and the lattice holds fewer nodes).  The
    projected fields agree within a few fp32 roundings of the largest near field; coordinates, dtypes and files are the same.
    ``exact_projection_device``: where angle and Cartesian projection monitors with ``far_field_approx=False`` take their surface
    integrals after the run — on the device in fp64 (True: ``fdtd_near_field``), in NumPy on the host (False), or per monitor (None: on
    the device from ``projection.EXACT_HOST_PAIRS`` point-node pairs on); ``SimulationData.log`` names the path per monitor.  With
    more than one GPU in ``devices`` the first one integrates.  ``rasterize_device``: paint Box, Sphere and Cylinder structures into
    the material volumes on the device during set-up (True; a scene with any other geometry, a Custom* medium, a Medium2D sheet or a
    medium of the whole-grid node lists takes the host path as a whole), on the host (False), or by
    ``discretize.RASTER_DEVICE_CELLS`` (None: the host); the volumes are the same bit for bit and ``SimulationData.log`` names the
    path.  One-GPU runs: with more than one GPU in ``devices`` every rank rasterises on the host, and True is refused.
    ``checkpoint``: the path of a state file; setting it turns checkpoint and resume on (docs/history/CHECKPOINT.md).  A file there
    that matches this call — the simulation, the number of steps, the device paths, the library — means the run continues from its
    time step (the log says ``Resumed from step S of N``); one that does not match raises ``SetupError`` and is left alone.
    ``checkpoint_steps``: write the file whenever the step count reaches a multiple of it.  ``step_budget`` / ``time_budget``: take
    at most that many time steps / start no new chunk of steps once that many seconds of solve time have passed in this call; a
    call that ends before the last step writes the file and raises ``exceptions.RunSuspended`` (``.path``, ``.step``) — the same
    call again resumes.  A call that reaches the last step, or stops on shutoff, removes the file and returns data that equal,
    bit for bit, those of the call without these keywords.  One-GPU runs; a budget or ``checkpoint_steps`` needs ``checkpoint``."""
    from .engine import HipEngine

    if checkpoint is None and any(v is not None for v in (checkpoint_steps, step_budget, time_budget)):
        raise Tidy3dNotImplementedError("checkpoint_steps / step_budget / time_budget without checkpoint= (the path of the state "
                                        "file) are not supported")
    if checkpoint_steps is not None and int(checkpoint_steps) < 1:
        raise Tidy3dNotImplementedError(f"checkpoint_steps={checkpoint_steps}: an interval below 1 time step is not supported")
    if checkpoint is not None and devices is not None and len(devices) > 1:
        raise Tidy3dNotImplementedError("checkpoint= together with devices= with more than one GPU is not supported (a z-slab run "
                                        "needs one state per rank)")
    sim, was_tidy3d = _as_mirror(simulation)
    sim = td.with_nonlinear(sim)      # (Medium placeholders with a NonlinearSpec of NonlinearSusceptibility models become media)
    sim.validate_pre_upload(source_required=True)
    paths = DevicePaths(flux_time_device, field_time_device, field_dft_device, projection_device)
    if devices is not None and len(devices) > 1:
        _device_refusals(sim, paths, "devices= with more than one GPU")
        if rasterize_device:
            raise Tidy3dNotImplementedError("rasterize_device=True (structures rasterised on the device) together with devices= with "
                                            "more than one GPU is not supported; rasterize_device=None or False keeps the host path")
        from .conformal import pec_conformal_of
        from .engine import refuse_together
        media = [m for m in sim.mediums if isinstance(m, td.Medium)]
        for kind, there, hint in (("modulation", any(m.is_time_modulated for m in media), ""),
                                  ("conformal", pec_conformal_of(sim) is not None, " (SubpixelSpec(pec=Staircasing()) is)"),
                                  ("nonlinear", any(m.is_nonlinear for m in media), "")):
            if there:     # (the whole-grid node lists the engine would refuse on its z-slabs, named before any worker starts)
                refuse_together(kind, "devices= with more than one GPU", hint)
        sim_data = _run_on_devices(sim, [int(d) for d in devices], n_steps, verbose,
                                   dict(_dist_options or {}, exact_projection_device=exact_projection_device))
        want_td = was_tidy3d if return_tidy3d is None else return_tidy3d
        if want_td:
            from .adapter import to_tidy3d
            out = to_tidy3d(sim_data, simulation if was_tidy3d else None)
            if path:
                out.to_file(path)
            return out
        if path:
            save(sim_data, path)
        return sim_data
    if devices is not None and len(devices) == 1:
        device = int(devices[0])
    t_setup = time.perf_counter()
    disc = discretize(sim, n_steps=n_steps, mode_grid_dispersion=mode_grid_dispersion, device_paths=paths,
                      rasterize_device=rasterize_device, lib=lib, gpu=device)
    spec = disc.spec
    lines = [f"Simulation domain Nx, Ny, Nz: {list(spec.shape)}",
             f"Applied symmetries: {tuple(sim.symmetry)}",
             f"Number of computational grid points: {spec.n_cells:.4e}.",
             f"Number of time steps: {spec.n_steps:.4e}",
             f"Time step size (dt): {spec.dt:.4e}s", "",
             "Running solver for %d time steps..." % spec.n_steps]
    if spec.raster_log:
        lines[-2:-2] = spec.raster_log.splitlines()
    if spec.conformal:
        lines.insert(-2, "PEC-conformal boundaries (Dey-Mittra): %d cut faces listed; single time steps."
                     % sum(len(cs.ijk) for cs in spec.conformal))

    if spec.nonlinear:
        lines.insert(-2, "Nonlinear (Kerr) media: %d nodes listed, %d fixed-point iterations per step; single time steps."
                     % (sum(len(ns.ijk) for ns in spec.nonlinear), spec.nonlinear[0].num_iters))

    def progress(step, t, decay):
        ln = _log_line(step, spec.n_steps, t, decay)
        lines.append(ln)
        if verbose:
            print(ln, flush=True)
        return False

    with HipEngine(spec, lib=lib, device=device) as eng:
        used_lib = eng.lib                                  # the library that ran the solve also integrates the projections
        setup_s = time.perf_counter() - t_setup
        t0 = time.perf_counter()
        if checkpoint is None:
            stats = eng.run(progress=progress if spec.decay_every else None)
            solve_s = time.perf_counter() - t0
        else:
            meta = _checkpoint_meta(sim, spec, mode_grid_dispersion, eng.lib)
            stats, solve_s = _run_in_chunks(eng, spec, progress if spec.decay_every else None, lines, verbose, str(checkpoint), meta,
                                            checkpoint_steps, step_budget, time_budget)
        raw = eng.results()
        from .projection import FLUX_SUFFIX
        raw.update({name + FLUX_SUFFIX: fl for name, fl in eng.lattice_flux().items()})    # DirectivityMonitor surfaces on the device path
        steps_done = int(stats.steps_done)
        diverged = bool(stats.diverged)
        if stats.stopped_early:
            lines.append(f"Field decay smaller than shutoff factor, exiting solver "
                         f"(time step {steps_done}).")
        if diverged:
            lines.append("WARNING: field divergence detected, exiting solver.")
        on_device = sorted({m.name.split("::")[0] for m in spec.monitors if m.kind == "flux_time"})
        gathered = sorted(m.name for m in spec.monitors if m.kind == "time_sparse")
        accumulated = sorted(m.name for m in spec.monitors if m.kind == "dft_sparse")
        on_lattice = sorted({m.name.split("::")[0] for m in spec.monitors if m.kind == "dft_lattice"})
        lines.append(schedule_line(stats, spec.n_cells, solve_s)
                     + (f" FluxTimeMonitor reduced on the device: {', '.join(on_device)}." if on_device else "")
                     + (f" FieldTimeMonitor gathered on the device: {', '.join(gathered)}." if gathered else "")
                     + (f" FieldMonitor accumulated on the device: {', '.join(accumulated)}." if accumulated else "")
                     + (f" Projection monitor accumulated on its lattice on the device: {', '.join(on_lattice)}." if on_lattice else ""))
    lines += ["", f"Setup time (s):  {setup_s:.4f}", f"Solver time (s): {solve_s:.4f}",
              f"Time-stepping speed (cells/s): {spec.n_cells * steps_done / max(solve_s, 1e-9):.2e}"]
    sim_data = assemble(disc, raw, log="\n".join(lines), diverged=diverged, n_steps_run=steps_done, device_lib=used_lib, device=device,
                        exact_projection_device=exact_projection_device)

    # post-run warnings, ref web/api/tidy3d_stub.py:219-233
    if diverged:
        log.warning("The simulation has diverged! For more information, check 'SimulationData.log'.")
    elif sim.shutoff != 0 and spec.decay_every and sim_data.final_decay_value > sim.shutoff:
        log.warning(f"Simulation final field decay value of {sim_data.final_decay_value} is greater "
                    f"than the simulation shutoff threshold of {sim.shutoff}. Consider running the "
                    "simulation again with a larger 'run_time' duration for more accurate results.")

    want_td = was_tidy3d if return_tidy3d is None else return_tidy3d
    if want_td:
        from .adapter import to_tidy3d
        out = to_tidy3d(sim_data, simulation if was_tidy3d else None)
        if path:
            out.to_file(path)
        return out
    if path:
        save(sim_data, path)
    return sim_data


def _run_on_devices(sim, devices, n_steps, verbose: bool, opt: dict) -> SimulationData:
    """Spawn one ``python -m tidy3d_amd.dist_main`` per GPU (ranks in the order of ``devices``; rendezvous on
    127.0.0.1), wait, and load what rank 0 wrote."""
    import pickle
    import socket
    import subprocess
    import sys
    import tempfile
    import time as _time
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    timeout_s = float(opt.get("timeout", 0) or 0)                 # whole multi-GPU call; 0 = none
    rdv_timeout = int(opt.get("rendezvous_timeout", 300))         # init_process_group of every rank
    with tempfile.TemporaryDirectory(prefix="tidy3d_amd_") as tmp:
        f_sim, f_out = os.path.join(tmp, "sim.pkl"), os.path.join(tmp, "data.pkl")
        with open(f_sim, "wb") as f:
            pickle.dump(sim, f, protocol=pickle.HIGHEST_PROTOCOL)
        # rank 0 binds the rendezvous port itself (MASTER_PORT=0 is not portable across torch versions), so the port is
        # chosen here — but held open until just before the ranks start, and a start that loses the race is retried
        for attempt in range(3):
            with socket.socket() as sck:
                sck.setsockopt(socket.SOL_SOCKET, socket.SO_REUSEADDR, 1)
                sck.bind(("127.0.0.1", 0))
                port = sck.getsockname()[1]
            procs, logs = [], []
            for rank, dev in enumerate(devices):
                env = dict(os.environ, RANK=str(rank), WORLD_SIZE=str(len(devices)), LOCAL_RANK=str(dev),
                           MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), TIDY3D_AMD_RDV_TIMEOUT=str(rdv_timeout))
                env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")       # dmabuf IPC (what this driver supports) unless the user chose
                env["PYTHONPATH"] = os.pathsep.join([root] + [p for p in (opt.get("pythonpath") or []) if p]
                                                    + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
                cmd = [sys.executable, "-m", "tidy3d_amd.dist_main", "--sim", f_sim, "--out", f_out,
                       "--backend", opt.get("backend", "nccl")]
                if n_steps is not None:
                    cmd += ["--n-steps", str(int(n_steps))]
                if opt.get("lib"):
                    cmd += ["--lib", opt["lib"]]
                if opt.get("hook"):
                    cmd += ["--hook", opt["hook"]]
                if opt.get("exact_projection_device") is not None:
                    cmd += ["--exact-projection-device", "on" if opt["exact_projection_device"] else "off"]
                # stderr goes to a FILE per rank: a pipe nobody drains blocks its rank after ~64 KiB (HIP / RCCL warnings,
                # AMD_LOG_LEVEL) — and with it every sibling waiting for that rank in a collective
                lf = open(os.path.join(tmp, f"rank{rank}.attempt{attempt}.err"), "w+")
                logs.append(lf)
                procs.append(subprocess.Popen(cmd, env=env, stdout=None if verbose else subprocess.DEVNULL, stderr=lf, text=True))
            # poll ALL ranks: the first one that fails takes its siblings down (they would otherwise sit in
            # init_process_group or in an RCCL send / recv for ever); an overall timeout does the same
            t0 = _time.monotonic()
            failed = None
            while True:
                codes = [p.poll() for p in procs]
                bad = [r for r, c in enumerate(codes) if c not in (None, 0)]
                if bad:
                    failed = (bad[0], codes[bad[0]])
                    break
                if all(c == 0 for c in codes):
                    break
                if timeout_s and _time.monotonic() - t0 > timeout_s:
                    failed = (-1, None)
                    break
                _time.sleep(0.05)
            if failed is not None:
                for p in procs:
                    if p.poll() is None:
                        p.terminate()
                for p in procs:
                    try:
                        p.wait(timeout=10)
                    except subprocess.TimeoutExpired:
                        p.kill()
                        p.wait()
            tails = []
            for lf in logs:
                lf.seek(0)
                tails.append(lf.read()[-2000:])
                lf.close()
            if failed is None:
                break
            r, rc = failed
            lost_port = r >= 0 and ("eaddrinuse" in tails[r].lower() or "address already in use" in tails[r].lower())
            if lost_port and attempt < 2:
                continue                                   # lost the race for the port: once more with another one
            if r < 0:
                raise SolverLibraryError(f"multi-GPU run: no result after {timeout_s:.0f} s (timeout); ranks terminated. "
                                         f"rank 0 stderr: {tails[0]}")
            raise SolverLibraryError(f"multi-GPU run: rank {r} exited with status {rc} (its siblings were terminated): {tails[r]}")
        with open(f_out, "rb") as f:
            return pickle.load(f)


def save(sim_data: SimulationData, path: str) -> None:
    """``.hdf5``: the reference's own file layout, written through the HDF5 C library
    (tidy3d_amd/hdf5io.py) — loadable with ``tidy3d.SimulationData.from_file``; anything else: .npz."""
    if path.endswith(".hdf5"):
        from .hdf5io import write_simulation_data
        write_simulation_data(sim_data, path)
    else:
        save_npz(sim_data, path)


def load(path: str) -> SimulationData:
    """Counterpart of ``tidy3d.web.load`` for a local file written by ``run(..., path=...)``."""
    from .hdf5io import load_simulation_data
    return load_simulation_data(path)


def save_npz(sim_data: SimulationData, path: str) -> None:
    """Plain .npz dump of every DataArray (values + coords) plus the log; the tidy3d hdf5
    container needs h5py and is written through the real package (adapter.to_tidy3d)."""
    blobs = {"log": np.array(sim_data.log or ""), "diverged": np.array(sim_data.diverged)}
    for d in sim_data.data:
        name = d.monitor.name
        arrays = getattr(d, "field_components", None)
        if arrays is None and hasattr(d, "amps"):
            arrays = {"amps": d.amps, "n_complex": d.n_complex}
            if getattr(d, "mode_power", None) is not None:
                arrays["mode_power"] = d.mode_power
        if arrays is None:
            arrays = {"flux": d.flux}
        for k, v in arrays.items():
            blobs[f"{name}/{k}"] = v.values
            for dim, c in v.coords.items():
                blobs[f"{name}/{k}/{dim}"] = c
    np.savez(path if path.endswith(".npz") else path + ".npz", **blobs)


# ----------------------------------------------------------------------------------------------
# Job / Batch façade (ref web/api/container.py): the cloud life cycle upload -> start -> monitor ->
# download -> load collapses to one local solve; names, arguments and return types are kept so that
# scripts written against tidy3d.web.Job / Batch run unchanged.
# ----------------------------------------------------------------------------------------------

DEFAULT_DATA_PATH = "simulation_data.hdf5"       # ref web/api/webapi.py / container.py defaults
DEFAULT_DATA_DIR = "."


class Job:
    """ref container.py:35 — one simulation; ``run(path)`` returns its SimulationData."""

    def __init__(self, simulation, task_name: str, folder_name: str = "default", callback_url: Optional[str] = None,
                 solver_version: Optional[str] = None, verbose: bool = True, simulation_type: str = "tidy3d",
                 parent_tasks=None, **run_kwargs):
        self.simulation, self.task_name, self.folder_name = simulation, task_name, folder_name
        self.verbose, self.run_kwargs = verbose, run_kwargs
        self.task_id = f"local-{task_name}"
        self._data: Optional[SimulationData] = None
        self._path: Optional[str] = None

    def upload(self) -> None:                       # nothing leaves this machine
        pass

    def start(self) -> None:
        if self._data is None:
            self._data = run(self.simulation, task_name=self.task_name, folder_name=self.folder_name,
                             verbose=self.verbose, **self.run_kwargs)

    def monitor(self) -> None:
        pass

    @property
    def status(self) -> str:
        return "success" if self._data is not None else "draft"

    def download(self, path: str = DEFAULT_DATA_PATH) -> None:
        self.start()
        data = self._data
        if hasattr(data, "to_file"):               # a genuine tidy3d.SimulationData
            data.to_file(path)
        else:
            save(data, path)
        self._path = path

    def load(self, path: str = DEFAULT_DATA_PATH):
        if self._data is None or self._path != path:
            self.download(path)
        return self._data

    def run(self, path: str = DEFAULT_DATA_PATH):
        """ref container.py:190-207."""
        self.upload()
        self.start()
        self.monitor()
        return self.load(path=path)

    def delete(self) -> None:
        self._data = None

    def estimate_cost(self, verbose: bool = True) -> float:
        return 0.0                                   # no FlexCredits on your own GPU

    real_cost = estimate_cost


class BatchData:
    """ref container.py:342 — maps task names to data files and loads them one at a time."""

    def __init__(self, task_paths: dict, task_ids: dict, verbose: bool = True, _cache: Optional[dict] = None):
        self.task_paths, self.task_ids, self.verbose = dict(task_paths), dict(task_ids), verbose
        self._cache = _cache or {}

    def load_sim_data(self, task_name: str):
        if task_name in self._cache:
            return self._cache[task_name]
        return load(self.task_paths[task_name])

    def items(self):
        for task_name in self.task_paths:
            yield task_name, self.load_sim_data(task_name)

    def __getitem__(self, task_name: str):
        return self.load_sim_data(task_name)

    def __len__(self):
        return len(self.task_paths)


class Batch:
    """ref container.py:426 — several simulations; ``run(path_dir)`` returns a BatchData.  The jobs
    run one after the other on the local GPU (``device=`` in ``run_kwargs`` selects it)."""

    def __init__(self, simulations: dict, folder_name: str = "default", verbose: bool = True,
                 solver_version: Optional[str] = None, callback_url: Optional[str] = None,
                 simulation_type: str = "tidy3d", parent_tasks=None, **run_kwargs):
        self.simulations, self.folder_name, self.verbose = dict(simulations), folder_name, verbose
        self.run_kwargs = run_kwargs
        self.jobs = {name: Job(sim, task_name=name, folder_name=folder_name, verbose=verbose, **run_kwargs)
                     for name, sim in self.simulations.items()}

    @property
    def num_jobs(self) -> int:
        return len(self.jobs)

    def upload(self) -> None:
        pass

    def start(self) -> None:
        for job in self.jobs.values():
            job.start()

    def monitor(self) -> None:
        pass

    @staticmethod
    def _job_data_path(task_id: str, path_dir: str = DEFAULT_DATA_DIR) -> str:
        return os.path.join(path_dir, f"{task_id}.hdf5")          # ref container.py:762-778

    def download(self, path_dir: str = DEFAULT_DATA_DIR) -> None:
        os.makedirs(path_dir, exist_ok=True)
        for job in self.jobs.values():
            job.download(self._job_data_path(job.task_id, path_dir))

    def load(self, path_dir: str = DEFAULT_DATA_DIR) -> BatchData:
        paths = {name: self._job_data_path(job.task_id, path_dir) for name, job in self.jobs.items()}
        for name, job in self.jobs.items():
            if job._path != paths[name]:
                job.download(paths[name])
        return BatchData(task_paths=paths, task_ids={n: j.task_id for n, j in self.jobs.items()},
                         verbose=self.verbose, _cache={n: j._data for n, j in self.jobs.items()})

    def run(self, path_dir: str = DEFAULT_DATA_DIR) -> BatchData:
        """ref container.py:523-557."""
        os.makedirs(path_dir, exist_ok=True)
        self.upload()
        self.start()
        self.monitor()
        self.download(path_dir=path_dir)
        return self.load(path_dir=path_dir)

    def delete(self) -> None:
        for job in self.jobs.values():
            job.delete()

    def estimate_cost(self, verbose: bool = True) -> float:
        return 0.0

    real_cost = estimate_cost
