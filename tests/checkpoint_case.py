"""Checkpoint and resume (docs/history/CHECKPOINT.md): the scenarios and the harness tests/test_emu_checkpoint.py and
tests/test_gpu_checkpoint.py share.

For every scenario the reference is a fresh handle that runs N steps in one call.  The subject runs k steps, its state is taken
(`HipEngine.get_state`, or a file of `save_state`), the handle is destroyed, and a fresh handle of the same spec — which has never
run — takes the state and runs the remaining N - k.  All six fields, every monitor array, the lattice fluxes and the four run
figures (steps_done, stopped_early, field_decay, diverged) must be equal bit for bit: there is no tolerance in this module.

Scenarios are the smallest grids on which each state section exists (the table of CHECKPOINT.md): each returns a `Case`."""
import dataclasses
from typing import Callable, Optional

import numpy as np

import tidy3d_amd.schema as td
from tidy3d_amd import lib as L
from tidy3d_amd.discretize import discretize
from tidy3d_amd.engine import HipEngine

import cases
import field_time_case as fieldtc
import flux_time_case as fluxtc
import test_emu_lifecycle as lc
from cases import DL, PULSE

STAT_KEYS = ("steps_done", "stopped_early", "field_decay", "diverged")
FUSED = {"variant": L.VARIANT_FUSED, "z_chunk": 2}
AUTO = {"variant": L.VARIANT_AUTO, "z_chunk": 0}
TWOPASS = {"variant": L.VARIANT_ZMARCH, "z_chunk": 2}


@dataclasses.dataclass
class Case:
    spec: object
    n: int                              # steps of the whole run
    ks: tuple                           # cut steps
    opts: dict = dataclasses.field(default_factory=dict)        # fdtd_set_option settings of the fused variant
    seed: Optional[int] = None          # random initial fields (the subject's first handle and the reference; never the resumed handle)
    kw: dict = dataclasses.field(default_factory=lambda: dict(FUSED))       # HipEngine keywords of the fused variant
    two_pass: bool = True               # the scenario also runs on the two-pass kernels
    proof: Optional[Callable] = None    # proof(rows: counters of the subject's two runs, engine of the second run)
    bloch: bool = False                 # a (re, im) pair of handles: HipEngine decides the variant and the layout


def engine(case, lib, variant, seed=None):
    if case.bloch:
        e = HipEngine(case.spec, lib=lib)
        assert e.twin is not None
    elif variant == "twopass":
        e = lc.engine(case.spec, lib, {}, None, **TWOPASS)
    else:
        e = lc.engine(case.spec, lib, case.opts, None, **case.kw)
    if seed is not None:
        lc.seed_fields(e, seed)
    return e


def snapshot(e):
    fields, results = lc.snapshot(e)
    results = dict(results)
    results.update({"lattice_flux::" + k: v for k, v in e.lattice_flux().items()})
    return fields, results


def uncut(case, lib, variant):
    """the reference: one handle, N steps in one call -> (fields, records, stats)"""
    with engine(case, lib, variant, case.seed) as e:
        st = e.run(case.n)
        return snapshot(e) + (st,)


def same_run(ref, got, st):
    lc.same(ref, got)
    for key in STAT_KEYS:
        assert getattr(st, key) == getattr(ref[2], key), (key, getattr(st, key), getattr(ref[2], key))


def cut_and_resumed(case, lib, variant, k, path=None, meta=None):
    """k steps on one handle, the state out (a blob, or the file `path`), the handle destroyed; a fresh handle that has not run takes it and
    runs to N -> (fields, records), stats, [counters of the two runs], the blob's bytes"""
    with engine(case, lib, variant, case.seed) as e:
        rows = [lc.counters(e, e.run(k))]
        fp = e.state_fingerprint()
        if path is None:
            blobs = [e.get_state()] + ([e.twin.get_state()] if e.twin is not None else [])
            assert int(e.seam_stats().seam_pending) == 0
        else:
            assert e.save_state(path, meta or {}) == rows[0]["steps_done"]
    n_bytes = None
    with engine(case, lib, variant) as e:
        assert int(e.stats().steps_done) == 0 and e.state_fingerprint() == fp
        if path is None:
            e.set_state(blobs[0])
            if e.twin is not None:
                e.twin.set_state(blobs[1])
            n_bytes = sum(int(b.nbytes) for b in blobs)
        else:
            e.load_state(path, meta or {})
        assert int(e.stats().steps_done) == rows[0]["steps_done"]
        st = e.stats()
        if not st.stopped_early and rows[0]["steps_done"] < case.n:
            st = e.run(case.n - rows[0]["steps_done"])
        rows.append(lc.counters(e, st))
        if case.proof:
            case.proof(rows, e)
        return snapshot(e), st, rows, n_bytes


def check(name, case, lib, variant, k):
    ref = uncut(case, lib, variant)
    got, st, rows, n_bytes = cut_and_resumed(case, lib, variant, k)
    lc.show(f"checkpoint {name} [{variant}] cut at {k} of {case.n} ({n_bytes} state bytes)", rows)
    same_run(ref, got, st)
    return rows


# ------------------------------------------------------------------------------------------------------------------- scenarios
def _pml_lorentz_sim(monitors=None, conductivity=0.0, sources=None):
    """24 x 20 x 28 cells with four CPML layers on all six faces inside them, a Lorentz block, a dipole"""
    body = [td.Structure(geometry=td.Box(center=(0.1, -0.05, 0.1), size=(0.3, 0.25, 0.3)), medium=td.Lorentz(eps_inf=2.0, coeffs=[(2.0, 4e14, 2e13)]))]
    if conductivity:
        body.append(td.Structure(geometry=td.Box(center=(0, 0, 0), size=(td.inf, td.inf, td.inf)), medium=td.Medium(permittivity=1.0, conductivity=conductivity)))
        body.reverse()
    N = (24 - 8, 20 - 8, 28 - 8)
    sim = cases._sim(N, td.BoundarySpec.all_sides(td.PML(num_layers=4)), body, monitors=monitors,
                     sources=sources or [td.PointDipole(center=(0.03, -0.07, 0.01), source_time=PULSE, polarization="Ez")])
    return dataclasses.replace(sim, size=tuple((n - 1e-6) * DL for n in N))      # (exactly N cells between the layers)


def scenario_a(n=7, ks=(3,)):
    """CPML psi on six faces, ADE e_old / q (unpaged at this size), time and DFT monitors; odd and even cuts"""
    spec = lc.spec_of(_pml_lorentz_sim(), n)
    assert spec.shape == (24, 20, 28) and any(m.poles for m in spec.media)
    return Case(spec, n, ks, {L.OPT_ROWS: 3, L.OPT_PML_SPLIT: 1, L.OPT_TWOSTEP: lc.W5, L.OPT_SHELL_PAIRS: 1, L.OPT_SHELL2: 1}, seed=3)


def scenario_a_pairs(n=16, ks=(6, 5)):
    """CPML on a grid whose shell is small enough for shell2 pairs (tests/test_emu_shell2.py's one-tile grid): both psi sides ping-pong
    between their sets inside the pairs.  k = 6 cuts behind an ODD number of pairs — the live psi lies in the arrays that were
    allocated second, the resumed handle puts it into the ones allocated first — and k = 5 behind two pairs and a single step"""
    spec = lc._shell_spec(n)

    def proof(rows, e):
        assert rows[0]["shell2_pairs"] > 0 and rows[1]["shell2_pairs"] > 0, rows

    return Case(spec, n, ks, {L.OPT_ROWS: 3, L.OPT_PML_SPLIT: 1, L.OPT_TWOSTEP: lc.W5, L.OPT_SHELL_PAIRS: 1, L.OPT_SHELL2: 1}, seed=7, proof=proof)


def live_round_trip(case, lib, variant="fused"):
    """get_state -> set_state on the SAME handle in mid-run (k steps, out, in, the rest): no bit of the rest changes, and the blob
    read back equals the one put in"""
    ref = uncut(case, lib, variant)
    k = case.ks[0]
    with engine(case, lib, variant, case.seed) as e:
        rows = [lc.counters(e, e.run(k))]
        blob = e.get_state()
        e.set_state(blob)
        assert np.array_equal(e.get_state(), blob)
        st = e.run(case.n - k)
        rows.append(lc.counters(e, st))
        if case.proof:
            case.proof(rows, e)
        same_run(ref, snapshot(e), st)
    return rows


def scenario_b(where):
    """two x tiles (emulator: 264 x 8 x 12; device: 520 x 96 x 72), plain pairs with deferred seam repair, a body across the seam,
    k odd: the cut falls where a pair — and a deferred repair — would have been"""
    from test_emu_seam_defer import TWO
    from test_emu_fused2 import MEDIA, _sim
    if where == "gpu":
        from test_gpu_seam_defer import BAR, _sim as big_sim
        spec, opts, kw, n, k = lc.spec_of(big_sim(structures=BAR), 12), {L.OPT_PLACEMENT_TRIES: 0, L.OPT_TWOSTEP: lc.W16, L.OPT_SEAM_DEFER: 1}, dict(FUSED, z_chunk=0), 12, 5
        assert spec.shape[0] > 512 and spec.shape[0] % 4 == 0      # (three x tiles: the grid of tests/test_gpu_lifecycle.py)
    else:
        spec, opts, kw, n, k = lc.spec_of(_sim(TWO, monitors=False, structures=MEDIA), 12), {L.OPT_ROWS: 3, L.OPT_TWOSTEP: lc.W16, L.OPT_SEAM_DEFER: 1}, dict(FUSED), 12, 5
        assert spec.shape[0] > 256

    def proof(rows, e):
        assert rows[0]["fused2_pairs"] > 0 and rows[1]["fused2_pairs"] > 0 and rows[0]["seam_deferred_pairs"] > 0, rows

    return Case(spec, n, (k,), opts, seed=5, kw=kw, proof=proof)


def scenario_c(oblique):
    """TFSF box (normal / oblique incidence): the incident lines e1 / h1, cut at the step of largest injection"""
    import source_state as ss
    sim = cases.tfsf_angled_box() if oblique else cases.tfsf_box()
    spec = lc.spec_of(sim, 110)
    inj = ss.injections(spec)[("TFSF box", 0, "E")]
    k = int(np.argmax(inj))
    assert 0 < k < 104 and inj[k] > 0, k
    n = k + 6
    return Case(spec, n, (k,), {L.OPT_ROWS: 3, L.OPT_TWOSTEP: lc.W5}, two_pass=True)


def scenario_d(where):
    """dispersive bodies advanced inside the pairs (disp.state == 1: disp_pairs > 0 in both runs): the paged memory terms of a handle
    that has not run yet are rebuilt from the restored pole states by its first run"""
    if where == "gpu":
        fn = cases.lorentz_sphere
        spec = lc.spec_of(fn(tuple(3 * n for n in fn.__defaults__[0])), 16)
        opts, kw = {L.OPT_PLACEMENT_TRIES: 0, L.OPT_TWOSTEP: 8 + 64 * 8, L.OPT_SHELL_PAIRS: 1, L.OPT_SHELL2: 1}, dict(FUSED, z_chunk=0)
    else:
        spec, opts, kw = lc._disp_spec(16), {L.OPT_ROWS: 3, L.OPT_TWOSTEP: lc.W16}, dict(FUSED)

    def proof(rows, e):
        assert rows[0]["disp_pairs"] > 0 and rows[1]["disp_pairs"] > 0, rows

    return Case(spec, 16, (7,), opts, kw=kw, proof=proof, two_pass=False)


def scenario_d_live(where):
    """the same scenario, the state put back into the LIVE handle that has paged: fdtd_set_state rebuilds the memory terms itself"""
    return scenario_d(where)


E_KINDS = {"time", "dft", "flux_time", "time_sparse", "dft_sparse", "dft_lattice"}


def scenario_e(n=24, k=11):
    """one monitor of every kind on 28 x 24 x 24 cells: whole-box time and DFT records, a flux-time surface and a sparse field-time
    monitor with rings of three records (part full at the cut, records on both sides of it), a sparse DFT monitor, and the lattices
    of a DirectivityMonitor (lattice DFT with flux weights)"""
    dt = discretize(cases._sim((20, 16, 16), td.BoundarySpec.all_sides(td.PML(num_layers=4)), monitors=[]), n_steps=4).spec.dt
    mons = [td.FieldTimeMonitor(center=(0.05, 0.0, 0.05), size=(0.4, 0.3, 0.3), name="t", interval=2, start=2.5 * dt, interval_space=(2, 2, 1)),
            td.FieldMonitor(center=(0, 0, 0), size=(0.5, 0.4, 0), freqs=[2.5e14, 3e14], name="f", interval_space=(2, 1, 1)),
            td.FluxTimeMonitor(center=(0.2, 0, 0), size=(0, 0.4, 0.4), name="ft", interval=2, start=2.5 * dt),
            td.DirectivityMonitor(name="dir", center=(0, 0, 0), size=(0.5, 0.4, 0.4), freqs=(2.7e14,), theta=(0.3, 1.2), phi=(0.0, 1.0), proj_distance=1e4)]
    sim = cases._sim((20, 16, 16), td.BoundarySpec.all_sides(td.PML(num_layers=4)), monitors=mons)
    on = dict(flux_time_device=True, field_time_device=True, field_dft_device=True, projection_device=True)
    dev = discretize(sim, n_steps=n, **on).spec
    host = discretize(sim, n_steps=n, **{key: False for key in on}).spec
    extra = [dataclasses.replace(m, name="host::" + m.name) for m in host.monitors if m.kind in ("time", "dft") and not m.name.startswith("dir")]
    spec = dataclasses.replace(dev, monitors=list(dev.monitors) + extra)
    spec = fieldtc.with_budget(fluxtc.with_budget(spec, 3), 3)
    spec.decay_every = 0
    kinds = {m.kind for m in spec.monitors}
    assert kinds == E_KINDS, kinds
    assert any(m.kind == "dft_lattice" and m.weights is not None for m in spec.monitors)
    for m in spec.monitors:
        if m.kind in ("time", "flux_time", "time_sparse"):
            before = sum(1 for s in m.steps if s < k)
            assert 0 < before < len(m.steps) and before % 3 != 0, (m.name, before)      # records on both sides of the cut, the ring part full
    assert all(dim <= lim for dim, lim in zip(spec.shape, (32, 24, 40)))
    return Case(spec, n, (k,), {L.OPT_ROWS: 3, L.OPT_PML_SPLIT: 1, L.OPT_TWOSTEP: lc.W5, L.OPT_SHELL_PAIRS: 1, L.OPT_SHELL2: 1})


def scenario_f(n=12, k=5):
    """Bloch cell with a fully anisotropic body cut by both wraps: the pair of handles, each with its own blob, the ghost-cell layout"""
    from test_aniso_bloch import wrapped_cell
    spec = lc.spec_of(wrapped_cell(), n)
    assert spec.bloch is not None and spec.aniso
    return Case(spec, n, (k,), bloch=True, two_pass=False)


def scenario_g(kind, n=7, k=3):
    """a modulation / PEC-conformal / Kerr list (the smallest scenario of its *_case module): the lists carry no state of their own —
    the fields and the step counter (the modulation's phase) suffice.  Random initial fields: the Kerr term is not small."""
    import modulation_case
    import nonlinear_case
    import pec_conformal_case
    if kind == "modulation":
        spec = modulation_case.small_at_wall()
        assert spec.modulation
    elif kind == "conformal":
        spec = pec_conformal_case.small_at_wall()
        assert spec.conformal
    else:
        spec = nonlinear_case.with_lists(nonlinear_case.small_at_wall(), scale=2e4)      # (chi3 I / eps_bar of a few per cent on fields of 1e-3)
        assert spec.nonlinear
    assert spec.n_steps >= n

    def proof(rows, e):
        assert all(c["fused2_pairs"] == 0 for c in rows), rows

    return Case(spec, n, (k,), seed=9, kw=dict(AUTO), proof=proof)


def scenario_h():
    """shutoff: random fields in a lossy CPML box only decay, a check every 4 steps stops the run early; cuts before the reference step
    of the shutoff, between two checks, and exactly on a check"""
    spec = lc.spec_of(_pml_lorentz_sim(conductivity=0.6), 60)
    spec.sources = []
    spec.decay_every, spec.shutoff, spec.decay_ref_step = 4, 0.9, 14
    assert spec.shape == (24, 20, 28)
    return Case(spec, 60, (3, 9, 8), {L.OPT_ROWS: 3, L.OPT_PML_SPLIT: 1, L.OPT_TWOSTEP: lc.W5, L.OPT_SHELL_PAIRS: 1, L.OPT_SHELL2: 1}, seed=11)


# ------------------------------------------------------------------------------------------------------------- web.run scenes
def web_scene(run_time=3e-14):
    """a FieldMonitor, a FluxTimeMonitor and a ModeMonitor behind a slab waveguide; a lossy background so that the shutoff is reached"""
    wg = td.Structure(geometry=td.Box(center=(0, 0, 0), size=(td.inf, 0.3, 0.25)), medium=td.Medium(permittivity=4.0))
    mons = [td.FieldMonitor(center=(0, 0, 0), size=(0.6, 0.5, 0), freqs=[3e14], name="field"),
            td.FluxTimeMonitor(center=(0.25, 0, 0), size=(0, 0.5, 0.5), name="flux_t", interval=2),
            td.ModeMonitor(center=(0.3, 0, 0), size=(0, 0.6, 0.5), freqs=[3e14], mode_spec=td.ModeSpec(num_modes=1), name="mode")]
    return td.Simulation(size=(1.0, 0.8, 0.7), grid_spec=td.GridSpec.uniform(dl=DL), run_time=run_time, structures=[wg],
                         sources=[td.PointDipole(center=(-0.2, 0, 0), source_time=PULSE, polarization="Ez")], monitors=mons,
                         boundary_spec=td.BoundarySpec.all_sides(td.PML(num_layers=4)), shutoff=0)


def same_data(a, b):
    """two SimulationData: every monitor's arrays, equal bit for bit"""
    assert set(a.monitor_data) == set(b.monitor_data)
    n = 0
    for name in a.monitor_data:
        da, db = a.monitor_data[name], b.monitor_data[name]
        for key, va in vars(da).items():
            vals = getattr(va, "values", va)
            if isinstance(vals, np.ndarray) and vals.dtype.kind in "fc":
                other = getattr(vars(db)[key], "values", vars(db)[key])
                assert np.array_equal(vals, other), (name, key)
                n += 1
    assert n > 0
    return n
