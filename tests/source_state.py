"""Live source injection held to the fp64 oracle node by node: the helper shared by tests/test_emu_source_state.py (emulator) and
tests/test_gpu_source_state.py (device), built on tests/dense_state.py.  docs/history/SOURCE_STATE.md holds the figures.

The dense-state suite starts at step 0, where a GaussianPulse(offset=5) stands at 4e-6 of its peak and the TFSF incident line holds
zeros: the sources are in its specs and add nothing a node-wise measure can see.  Here they are live:

  warm-up  both sides take W steps from zero fields; W is the step at which the case's largest single-step injection happens (the value
           point_source_kernel / tfsf_corr_kernel adds at a node, H x eta0), found from the fp64 oracle alone (``injections``)
  state    all six fields are then overwritten on both sides with dense_state's state of amplitude A = the largest single-step injection
           over steps W .. W + 5; the incident lines, psi and the pole states stay as the warm-up left them
  measure  K = 1, 2 and 6 more steps, dense_state.measure unchanged, through dense_state.PATHS
  floor    the same protocol between OracleFdtd(spec, dtype=np.float32) and the fp64 oracle; bar = dense_state.MARGIN x floor
  asserted from the fp64 oracle alone, before an engine runs: every list (each side of it) injects 0.1 A or more at some step of the
           window (a list that is meant to be spent: up to its last step); no listed node is excluded."""
import dataclasses

import numpy as np

import tidy3d_amd.schema as td
from tidy3d_amd import lib as L
from tidy3d_amd.discretize import discretize

import cases
import dense_state as ds

N_STEPS = 112                 # the waveforms' length: W + 8 or more in every scenario (asserted)
WINDOW = max(ds.KS)           # steps W .. W + 5
LIVE = 0.1                    # x A
ENDS = 3                      # a list that is meant to be spent ends at W + ENDS


# ---------------------------------------------------------------------------------------------------------------- injections
def injections(spec):
    """{(kind, list, side): [n_steps] the largest |value added at a node| by that side of that list at each step, H x eta0}, from the
    fp64 oracle alone: the point lists' products as ``OracleFdtd`` forms them, the boxes' from the incident lines of an oracle that
    runs from zero fields (the lines do not depend on the 3-D fields)."""
    from oracle.fdtd_numpy import OracleFdtd
    n, out = spec.n_steps, {}
    for q, s in enumerate(spec.sources):
        for side, wave, sel, unit in (("E", s.wave_e, s.comp < 3, 1.0), ("H", s.wave_h, s.comp >= 3, ds.ETA0)):
            if sel.any():
                z = (s.w_re[sel] + 1j * s.w_im[sel])[None, :] * np.asarray(wave)[:n, None]
                a = np.zeros(n)
                a[:len(z)] = unit * (np.abs(z) if spec.bloch is not None else np.abs(z.real)).max(axis=1)
                out[("point list", q, side)] = a
    if spec.tfsf:
        line = dataclasses.replace(spec, sources=[], monitors=[])
        o = OracleFdtd(line)
        for q, t in enumerate(spec.tfsf):
            out[("TFSF box", q, "E")], out[("TFSF box", q, "H")] = np.zeros(n), np.zeros(n)
        for step in range(n):
            e_now = [st["e"].copy() for st in o.tfsf_state]
            o._tfsf_h(step)
            for q, (t, st) in enumerate(zip(spec.tfsf, o.tfsf_state)):
                if step < len(t.wave):
                    out[("TFSF box", q, "H")][step] = ds.ETA0 * np.abs(t.h_corr_w * e_now[q][t.h_corr_aux]).max()
                    out[("TFSF box", q, "E")][step] = np.abs(t.e_corr_w * st["h"][t.e_corr_aux]).max()
            o._tfsf_e(step)
    return out


def last_step(spec, key):
    """the last step at which the list injects"""
    kind, q, side = key
    return (len(spec.tfsf[q].wave) if kind == "TFSF box" else len(spec.sources[q].wave_e if side == "E" else spec.sources[q].wave_h)) - 1


def listed_nodes(spec):
    """per component the boolean [nz, ny, nx] mask of the nodes some list holds"""
    nx, ny, nz = spec.shape
    out = [np.zeros((nz, ny, nx), bool) for _ in range(6)]
    lists = [(s.comp, s.ijk) for s in spec.sources]
    for t in spec.tfsf:
        lists += [(t.e_corr_comp, t.e_corr_ijk), (t.h_corr_comp, t.h_corr_ijk)]
    for comp, ijk in lists:
        for c in range(6):
            m = comp == c
            out[c][ijk[m, 2], ijk[m, 1], ijk[m, 0]] = True
    return out


# ---------------------------------------------------------------------------------------------------------------- the case
class SourceCase(ds.Case):
    """dense_state.Case behind a warm-up of W steps, with the state's amplitude taken from the injections; the conditions on the
    reference are asserted when the case is built.  ``engine``: keywords for dense_state.run_engine (z_chunk, options)."""
    tag = "source"

    def __init__(self, label, spec, seed=1, spent=(), engine=None):
        self.label, self.spec, self.engine = label, spec, dict(engine or {})
        self.inj = injections(spec)
        assert self.inj, label
        total = np.max(list(self.inj.values()), axis=0)
        self.warmup = self.W = int(np.argmax(total))
        assert spec.n_steps >= self.W + 8, (label, self.W, spec.n_steps)
        self.A = float(total[self.W:self.W + WINDOW].max())
        self.state, self.excluded = ds.admissible_state(spec, seed, amp=self.A)
        self.share = ds.excluded_share(self.excluded)
        self._ref, self._floor, self._f32 = {}, {}, {}
        self.note = f" | W {self.W} A {self.A:.3e}"
        # live: every side of every list, inside the window
        self.live = {}
        for key, a in self.inj.items():
            end = last_step(spec, key)
            assert (end < self.W + WINDOW) == (key[:2] in spent), (label, key, end, self.W)       # spent where it is meant to be, only there
            assert end >= self.W, (label, key, end)
            self.live[key] = float(a[self.W:min(self.W + WINDOW, end + 1)].max()) / self.A
            assert self.live[key] >= LIVE, f"{label}: {key} injects {self.live[key]:.3f} A at most over steps {self.W} .. {self.W + WINDOW - 1}"
        # counted: no listed node is excluded
        for c, (m, ex) in enumerate(zip(listed_nodes(spec), self.excluded)):
            assert not (m & ex).any(), f"{label}: {int((m & ex).sum())} listed {ds.COMP[c]} nodes are excluded"
        # only the oracle's pinned nodes and what lies beyond a PMC-plus wall are excluded: they are the zeros of the state
        for c in range(6):
            assert ((self.state[c] == 0) == self.excluded[c]).all(), (label, c)

    def ref(self, K):
        if not self._ref:
            self._ref = ds.run_oracle(self.spec, self.state, ds.KS, warmup=self.W)
        return self._ref[K]

    def floor(self, K):
        if K not in self._floor:
            if not self._f32:
                self._f32 = ds.run_oracle(self.spec, self.state, ds.KS, dtype=np.float32, warmup=self.W)
            self._floor[K] = ds.measure(self.spec, self.state, self.excluded, self.ref(K), self._f32[K])
        return self._floor[K]

    def bars(self, K):
        """every figure against 8 x its OWN floor: the records taken during the warm-up (little field yet, and outside a TFSF box what
        two large terms leave of each other) have a floor of their own that must not widen the nodes' bar"""
        f, r = self.floor(K)
        return ds.MARGIN * f.value, ds.MARGIN * r.value

    def run(self, lib, K, path, **kw):
        return ds.run_engine(self.spec, lib, self.state, K, path, warmup=self.W, **{**self.engine, **kw})

    def planted(self, K, plant):
        """the oracle with ``plant`` through the same protocol"""
        return ds.run_oracle(self.spec, self.state, K, plant=plant, warmup=self.W)


# ---------------------------------------------------------------------------------------------------------------- specs
def _finish(sim, n_steps=N_STEPS):
    spec = discretize(sim, n_steps=n_steps).spec
    spec.decay_every = 0
    return spec


def balanced(spec):
    """the point lists of ``spec`` with every side's weights scaled to the strongest side's peak injection (H x eta0): a unit magnetic
    dipole injects eta0 x less than a unit electric one in these units, which would leave its list at rest beside the other's"""
    inj = {k: v.max() for k, v in injections(dataclasses.replace(spec, tfsf=[])).items()}
    if not inj:
        return spec
    top = max(inj.values())
    out = []
    for q, s in enumerate(spec.sources):
        f = np.ones(len(s.comp))
        for side, sel in (("E", s.comp < 3), ("H", s.comp >= 3)):
            if sel.any():
                f[sel] = top / inj[("point list", q, side)]
        out.append(dataclasses.replace(s, w_re=s.w_re * f, w_im=s.w_im * f))
    spec.sources = out
    return spec


def case_spec(name, shape=None, n_steps=N_STEPS):
    return balanced(ds.case_spec(name, shape, n_steps=n_steps))


def one_list_spec():
    """``pec_box`` with its electric and its magnetic dipole in ONE list"""
    from test_emu_srcpaged import one_list
    spec = case_spec("pec_box")
    one_list(spec, 0, 1)
    assert len(spec.sources) == 1 and (spec.sources[0].comp < 3).any() and (spec.sources[0].comp >= 3).any()
    return spec


def _peak(a):
    return int(np.argmax(np.abs(a)))


def _delayed(wave, by):
    out = np.zeros_like(wave)
    out[by:] = wave[:len(wave) - by]
    return out


def dipole_on_box_spec():
    """``tfsf_box`` and an electric dipole whose strongest node is an Ez node on a vertical edge of the box, which both boxes of the
    polarisation angle correct: three lists meet there, the boxes add first, the dipole behind them.  The dipole's waveform is delayed to the step at which the box injects most and
    its weights are scaled to the box's injection, so that both lists are live in one window."""
    src = td.PointDipole(center=(0.03, -0.07, 0.01), source_time=cases.PULSE, polarization="Ez")
    sim = cases.tfsf_box()
    spec = _finish(dataclasses.replace(sim, sources=list(sim.sources) + [src]))
    (s,), (t0, t1) = spec.sources, spec.tfsf
    both = set(map(tuple, t0.e_corr_ijk[t0.e_corr_comp == 2].tolist())) & set(map(tuple, t1.e_corr_ijk[t1.e_corr_comp == 2].tolist()))
    target = np.asarray(sorted(both)[0])                   # an Ez node on a vertical edge of the box: both boxes correct it
    inj = injections(dataclasses.replace(spec, sources=[]))
    box = np.max(list(inj.values()), axis=0)
    own = np.abs(s.w_re).max() * np.abs(s.wave_e).max()
    by = _peak(box) - _peak(s.wave_e)
    assert by > 0
    spec.sources = [dataclasses.replace(s, ijk=(s.ijk + (target - s.ijk[_peak(s.w_re)])[None, :]).astype(s.ijk.dtype), w_re=s.w_re * box.max() / own,
                                        wave_e=_delayed(s.wave_e, by), wave_h=_delayed(s.wave_h, by), name="dipole on the box")]
    assert len(ds.listed(spec, 2, tuple(int(v) for v in target))) == 3
    return spec


def two_sheets_spec():
    """two electric current sheets on ONE plane (same nodes, two lists), periodic across, CPML along the normal"""
    mk = lambda amp: td.UniformCurrentSource(center=(0, 0, -0.2), size=(td.inf, td.inf, 0), polarization="Ex",        # noqa: E731
                                             source_time=td.GaussianPulse(freq0=3e14, fwidth=1.5e14, amplitude=amp))
    bspec = td.BoundarySpec(x=td.Boundary.periodic(), y=td.Boundary.periodic(), z=td.Boundary.pml(num_layers=4))
    spec = _finish(cases._sim((12, 10, 16), bspec, sources=[mk(1.0), mk(0.6)]))
    a, b = spec.sources
    assert np.array_equal(a.ijk, b.ijk) and np.array_equal(a.comp, b.comp)
    return spec


def spent_box_spec():
    """``tfsf_box`` whose second box's waveform ends at W + 3: no corrections behind it and its incident line rests, the first goes on"""
    spec = case_spec("tfsf_box")
    W = SourceCase("probe", spec).W
    spec.tfsf = [spec.tfsf[0], dataclasses.replace(spec.tfsf[1], wave=spec.tfsf[1].wave[:W + ENDS + 1])]
    return spec


def spent_list_spec(ends=ENDS):
    """``pec_box`` whose first list's waveforms end at W + ``ends`` (``alive(n)``), the second list — magnetic nodes — goes on.  With
    ``ends`` = 3 and 2 the last step falls once on the first and once on the second step of a pair of the K = 6 run: a pair (n, n + 1)
    whose first step is a list's last must not take the other list's H-side terms of step n + 1 from the sweep's node table"""
    spec = case_spec("pec_box")
    W = SourceCase("probe", spec).W
    s = spec.sources[0]
    spec.sources = [dataclasses.replace(s, wave_e=s.wave_e[:W + ends + 1], wave_h=s.wave_h[:W + ends + 1])] + spec.sources[1:]
    assert (spec.sources[1].comp >= 3).all()
    return spec


def sheet_cpml_spec():
    """an electric current sheet of 20 x 16 cells normal to z (640 nodes: more than the sweep's node table holds) deep inside CPML on
    every face, at the size at which the run takes shell pairs: paged terms inside shell2 pairs, or — with FDTD_OPT_SRC_PAGED = 0 —
    shell pairs whose bulk leaves the sheet's planes to single steps (z holes)"""
    src = td.UniformCurrentSource(center=(0.0, 0.01, 0.23), size=(20 * cases.DL, 16 * cases.DL, 0), source_time=cases.PULSE, polarization="Ex")
    bspec = td.BoundarySpec(x=td.Boundary.pml(num_layers=4), y=td.Boundary.pml(num_layers=3), z=td.Boundary.pml(num_layers=3))
    spec = _finish(cases._sim((44, 30, 28), bspec, sources=[src]))
    assert len(spec.sources[0].comp) > 256
    return spec


def sheet_x264_spec():
    """an electric current sheet of 40 x 8 cells across column 256 of a 264-cell row, in PEC walls: paged terms on both x tiles"""
    N = (264, 16, 12)
    x0 = (-0.5 * N[0] + 250) * cases.DL
    src = td.UniformCurrentSource(center=(x0, 0.01, 0.03), size=(40 * cases.DL, 8 * cases.DL, 0), source_time=cases.PULSE, polarization="Ey")
    spec = _finish(cases._sim(N, td.BoundarySpec.all_sides(td.PECBoundary()), sources=[src]))
    i = spec.sources[0].ijk[:, 0]
    assert i.min() < ds.X_TILE - 2 and i.max() > ds.X_TILE + 2 and len(i) > 256, (i.min(), i.max(), len(i))
    return spec


Z_CHUNK = {"emu": 2, "gpu": 8}
# label -> (builder of the spec, the lists (kind, index) that are meant to be spent inside the window, engine keywords)
SCENARIOS = {
    **{n: ((lambda n=n: case_spec(n)), (), {}) for n in ("tfsf_box", "tfsf_angled_box", "planewave_periodic", "bloch_planewave", "pec_box",
                                                        "pmc_plus_mix", "two_d", "one_d")},
    "one_list_e_and_h": (one_list_spec, (), {}),
    "dipole_on_box": (dipole_on_box_spec, (), {}),
    "two_sheets_one_plane": (two_sheets_spec, (), {}),
    "spent_box": (spent_box_spec, (("TFSF box", 1),), {}),
    "spent_list": (spent_list_spec, (("point list", 0),), {}),
    "spent_list_even": ((lambda: spent_list_spec(ENDS - 1)), (("point list", 0),), {}),
    "tfsf_box_z_chunks": ((lambda: case_spec("tfsf_box")), (), {"z_chunk": Z_CHUNK}),
    "tfsf_box_x3": ((lambda: case_spec("tfsf_box", ds.times("tfsf_box"), n_steps=N_STEPS + 24)), (), {}),
    "sheet_x264": (sheet_x264_spec, (), {}),
    "sheet_cpml": (sheet_cpml_spec, (), {}),
    "sheet_cpml_unpaged": (sheet_cpml_spec, (), {"options": ((L.OPT_SRC_PAGED, 0),)}),
}
# label -> what its K = 6 run through "pairs" must show in the counters of that run (worked out on the emulator): step pairs, of them
# with paged source terms ("paged"), carried in the sweep's node table ("table": pairs, none of them paged), or with paging switched
# off and the lists' planes left to single steps ("holes": pairs, none of them paged, none in the shell2 form); "either": a pair that
# the node table must refuse goes out paged.  The rest keep single steps and say why in fused2_off_reason.
TAKES_PAIRS = {"pec_box": "table", "one_list_e_and_h": "table", "spent_list": "either", "spent_list_even": "either", "tfsf_box_x3": "paged",
               "sheet_x264": "paged", "sheet_cpml": "paged", "sheet_cpml_unpaged": "holes"}
_CASES = {}


def case(label, where="emu"):
    """the SourceCase of ``label``, built once per process; ``where`` ("emu" or "gpu") picks the engine keywords that differ between
    the two (the z chunk) for the copy handed out — state, references and floors are shared"""
    if label not in _CASES:
        build, spent, _ = SCENARIOS[label]
        _CASES[label] = SourceCase(label, build(), spent=spent)
    if (label, where) not in _CASES:
        import copy
        c = copy.copy(_CASES[label])
        c.engine = {k: (v[where] if isinstance(v, dict) else v) for k, v in SCENARIOS[label][2].items()}
        _CASES[(label, where)] = c
    return _CASES[(label, where)]


def engine_vs_oracle(label, path, lib, where, ks=ds.KS):
    """the scenario through ``path`` at every K: every node and record element under 8 x its floor, the counters of the K = 6 run"""
    c = case(label, where)
    for K in ks:
        if path == "pairs" and K == 1:
            continue
        got = c.run(lib, K, path)
        c.check(got, K, f"{path} {c.engine or ''}")
        if path != "pairs":
            assert got.pairs == 0
        elif K == 6 and label in TAKES_PAIRS:
            kind = TAKES_PAIRS[label]
            assert got.pairs >= 1 and got.why == 0, (label, got.pairs, got.why)
            assert kind == "either" or (got.src_paged_pairs > 0) == (kind == "paged"), (label, kind, got.pairs, got.src_paged_pairs)
            assert kind != "holes" or got.shell2_pairs == 0, (label, got.pairs, got.shell2_pairs)
    return got


# ---------------------------------------------------------------------------------------------------------------- planted deviations
def _with(o, **lists):
    """give the oracle instance a spec of its own with ``tfsf`` / ``sources`` replaced"""
    o.spec = dataclasses.replace(o.spec, **lists)


def plant_tfsf(box, rel=None, **edit):
    """``edit``: field -> (index, what): "rel" multiplies that entry by 1 + REL, "+1" moves an index by one"""
    def plant(o):
        t = o.spec.tfsf[box]
        new = {}
        for name, (i, what) in edit.items():
            a = np.array(getattr(t, name))
            a[i] = a[i] + 1 if what == "+1" else a[i] * (1.0 + ds.REL)
            new[name] = a
        _with(o, tfsf=[dataclasses.replace(t, **new) if q == box else x for q, x in enumerate(o.spec.tfsf)])
    return plant


def plant_list(q, drop_last=False, **edit):
    """``edit``: field -> index of the entry multiplied by 1 + REL; ``drop_last``: the list without its last entry"""
    def plant(o):
        s = o.spec.sources[q]
        new = {}
        for name, i in edit.items():
            a = np.array(getattr(s, name))
            a[i] = a[i] * (1.0 + ds.REL)
            new[name] = a
        if drop_last:
            new = {name: getattr(s, name)[:-1] for name in ("comp", "ijk", "w_re", "w_im")}
        _with(o, sources=[dataclasses.replace(s, **new) if r == q else x for r, x in enumerate(o.spec.sources)])
    return plant


def _edge_entry(t):
    """an entry of the E-side list on a node with the most entries (an edge of the box)"""
    key = np.concatenate([t.e_corr_comp[:, None], t.e_corr_ijk], axis=1)
    _, inv, count = np.unique(key, axis=0, return_inverse=True, return_counts=True)
    on_edge = np.nonzero(count[inv.reshape(-1)] == count.max())[0]
    return int(on_edge[np.argmax(np.abs(t.e_corr_w[on_edge]))]), int(count.max())


PLANT_IDS = ("e_corr_w_of_an_edge_node", "h_corr_aux_moved_by_one", "ah_and_be_of_an_aux_cell", "w_im_of_a_bloch_sheet_node",
             "w_re_of_the_last_entry", "last_entry_dropped", "wave_e_at_W_plus_1")


def plant_of(pid):
    """-> (scenario, K, plant, the clause the failure sentence must hold, the entry it must name or None, the aux index or None)"""
    if pid == "e_corr_w_of_an_edge_node":
        q, n = _edge_entry(case("tfsf_angled_box").spec.tfsf[0])
        assert n >= 8
        return "tfsf_angled_box", 1, plant_tfsf(0, e_corr_w=(q, "rel")), "TFSF box 0, E side", q, None
    if pid == "h_corr_aux_moved_by_one":
        box = case("tfsf_box").spec.tfsf[0]
        q = int(np.argmax(np.abs(box.h_corr_w)))
        return "tfsf_box", 1, plant_tfsf(0, h_corr_aux=(q, "+1")), "TFSF box 0, H side", q, int(box.h_corr_aux[q])
    if pid == "ah_and_be_of_an_aux_cell":
        # the LAST cell the box reads: the wave runs up the line, so what the plant does further down the line lies outside the box and
        # the worst node is one that reads the planted cell itself
        box = case("tfsf_box").spec.tfsf[0]
        i = int(min(box.e_corr_aux.max(), box.h_corr_aux.max()))
        assert box.src_cell < i and (box.e_corr_aux == i).any() and (box.h_corr_aux == i).any()
        return "tfsf_box", 1, plant_tfsf(0, ah=(i, "rel"), be=(i, "rel")), "TFSF box 0", None, i
    if pid == "w_im_of_a_bloch_sheet_node":
        q = int(np.argmax(np.abs(case("bloch_planewave").spec.sources[0].w_im)))
        return "bloch_planewave", 1, plant_list(0, w_im=q), "point list 0", q, None
    last = len(case("pec_box").spec.sources[0].comp) - 1
    if pid == "w_re_of_the_last_entry":
        return "pec_box", 1, plant_list(0, w_re=last), "point list 0", last, None
    if pid == "last_entry_dropped":
        return "pec_box", 1, plant_list(0, drop_last=True), "point list 0", last, None
    assert pid == "wave_e_at_W_plus_1", pid
    return "pec_box", 2, plant_list(0, wave_e=case("pec_box").W + 1), "point list 0", None, None


def named(at, clause):
    """-> (entries, aux indices) of the first "listed: ``clause`` ..." part of a failure sentence"""
    import re
    part = next(p for p in at.split("; ") if p.startswith("listed: " + clause))
    entries = [int(v) for v in re.search(r"entr(?:y|ies) ([\d, ]+) of ", part).group(1).split(", ")]
    aux = re.search(r"reading aux ([\d, ]+) of ", part)
    return entries, [int(v) for v in aux.group(1).split(", ")] if aux else []
